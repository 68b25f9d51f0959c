#!/bin/bash
# builds the round-10 lab variants (gfx950 cross-compile): tools/r10/lab/bin/<name>
cd "$(dirname "$0")" && mkdir -p bin
build() { src=$1; name=$2; shift 2; /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form -I ../../../include -DLAB_NAME="\"$name\"" "$@" $src -o bin/$name 2>&1 | grep -i "error" -A3; }
build w64_edges_lab.hip w64_base &
build w64_edges_lab.hip w64_edges -DMILE_LAB_W64_EDGES &
build w64_edges_lab.hip w64_plain -DMILE_LAB_W64_STORE=0 &
build w64_edges_lab.hip w64_nt -DMILE_LAB_W64_STORE=2 &
build upd_edges_lab.hip upd_base &
build upd_edges_lab.hip upd_edges -DMILE_LAB_UPD_EDGES &
wait
ls bin
