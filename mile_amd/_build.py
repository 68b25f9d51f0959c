"""Build libmile_hip.so in-tree with hipcc for gfx950 (MI355X).

The .so is git-ignored but travels to the GPU box with the gpurun snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
CSRC = PKG_DIR / 'csrc'
LIB_PATH = PKG_DIR / 'libmile_hip.so'
# translation units and their extra flags.  -amdgpu-mfma-vgpr-form: MFMA results that the VALU consumes next land in VGPRs
# instead of AGPRs (fewer v_accvgpr moves and spills in the register-bound grad kernels; measured +0.5 % w64, +2 % w128b);
# mile_w64_fq2.hip is built without it (hipcc 7.2 crashes on k_grad_w64<3,2,true> with it).
VGPR_FORM = ['-mllvm', '-amdgpu-mfma-vgpr-form']
SOURCES = {'mile_hip.hip': VGPR_FORM, 'mile_eval.hip': [], 'mile_w64_fq2.hip': [], 'mile_narrow_part.hip': VGPR_FORM, 'mile_lenetti.hip': [], 'mile_attn.hip': [], 'mile_attn_pre.hip': [], 'mile_attn_wide.hip': [], 'mile_diag.hip': [], 'mile_fdiag.hip': [], 'mile_dtail.hip': [], 'mile_moments.hip': [], 'mile_lppd.hip': [], 'mile_quantiles.hip': [], 'mile_loo.hip': [], 'mile_lxp.hip': [], 'mile_calib.hip': [], 'mile_stack.hip': [], 'mile_crps.hip': [], 'mile_canon.hip': [], 'mile_align.hip': [], 'mile_sens.hip': [], 'mile_pdp.hip': []}
HEADERS = ['mile_device.h', 'mile_block.h', 'mile_grad_generic.h', 'mile_grad_narrow.h', 'mile_grad_w64.h', 'mile_grad_w64_block.inc', 'mile_bf16_frag.h',
           'mile_grad_w128b.h', 'mile_grad_gemm.h', 'mile_mm3.h', 'mile_lenet.h', 'mile_lenet_mfma.h', 'mile_lenetti.h', 'mile_attn.h', 'mile_attn_pre.h', 'mile_attn_wide.h', 'mile_predict.h', 'mile_row_head.h', 'mile_update.h', 'mile_diag.h', 'mile_diag_device.h', 'mile_fdiag.h', 'mile_dtail.h', 'mile_moments.h', 'mile_lppd.h', 'mile_quantiles.h', 'mile_loo.h', 'mile_loo_device.h', 'mile_lxp.h', 'mile_calib.h', 'mile_stack.h', 'mile_crps.h', 'mile_canon.h', 'mile_align.h', 'mile_sens.h', 'mile_chan.h', 'mile_pdp.h', 'mile_eval_plan.h', 'mile_eval_handle.h', 'mile_layer_plan.h']
OBJ_DIR = PKG_DIR / 'csrc' / '_obj'


def _hipcc() -> str:
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError('hipcc not found: libmile_hip.so cannot be built')


def _obj(src: str) -> Path:
    return OBJ_DIR / (Path(src).stem + '.o')


def _stale(src: str) -> bool:
    """Is the unit's source, any header, include/mile_hip.h or this file newer than its object?  No dependency scanning.  Where
    the object is not there (a tree that received the .so without the objects) the .so stands in for it."""
    product = _obj(src) if _obj(src).exists() else LIB_PATH
    deps = [CSRC / f for f in [src] + HEADERS] + [PKG_DIR.parent / 'include' / 'mile_hip.h', Path(__file__).resolve()]
    return not product.exists() or any(p.stat().st_mtime > product.stat().st_mtime for p in deps)


def needs_build() -> bool:
    return not LIB_PATH.exists() or any(_stale(src) for src in SOURCES)


def build_library(force: bool = False, verbose: bool = False) -> Path:
    """hipcc --offload-arch=gfx950: one object per translation unit (compiled concurrently), then
    -shared -> mile_amd/libmile_hip.so.  Without `force` only the stale units compile (and, as the link needs every object,
    those whose object is missing); MILE_HIPCC_FLAGS compiles all."""
    extra = os.environ.get('MILE_HIPCC_FLAGS', '').split()          # dev: extra compiler flags for experiments
    units = [src for src in SOURCES if force or extra or _stale(src)]
    if not units and LIB_PATH.exists():
        return LIB_PATH
    OBJ_DIR.mkdir(exist_ok=True)
    units += [src for src in SOURCES if src not in units and not _obj(src).exists()]
    base = [_hipcc(), '-O3', '--offload-arch=gfx950', '-std=c++17', '-fPIC']
    jobs = []
    for src in units:
        flags, obj = SOURCES[src], _obj(src)
        cmd = base + flags + extra + ['-c', str(CSRC / src), '-o', str(obj)]
        if verbose:
            print(' '.join(cmd))
        jobs.append((src, obj, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for src, obj, proc in jobs:
        out, err = proc.communicate()
        if proc.returncode != 0:
            for _, _, other in jobs:
                if other.poll() is None:
                    other.kill()
            for _, o, _ in jobs:                                      # no object of this run outlives its failure
                o.unlink(missing_ok=True)
            raise RuntimeError(f'hipcc failed on {src}:\n{out}\n{err}')
    link = [_hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-o', str(LIB_PATH)] + [str(_obj(src)) for src in SOURCES] + ['-ldl']
    if verbose:
        print(' '.join(link))
    res = subprocess.run(link, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f'hipcc link failed:\n{res.stdout}\n{res.stderr}')
    return LIB_PATH


if __name__ == '__main__':
    print(build_library(force=True, verbose=True))
