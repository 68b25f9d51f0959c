"""Writes the digests tests/test_gpu_w64_edges.py compares with (w64_edges_parent.json), from whatever build is imported.

The committed file was written by this script on an MI355X from a checkout of the commit BEFORE the k_grad_w64 staging was
pipelined and its slab stores made write-through (`git log -- mile_amd/csrc/mile_grad_w64.h`), with that commit's library:

    git worktree add ../before <that commit> && (cd ../before && python __graft_entry__.py)
    cd ../before && python <this checkout>/tests/golden/make_w64_edges_digests.py out.json

It takes mile_amd and the oracle from the current directory and the cases, the launch and the digest from the test module next
to it, so the reference side and the tested side run the same inputs through the same code.  Regenerate only from a build whose
slabs are known good: the digests are the reference, not a property of the inputs.
"""
import importlib.util
import json
import sys
from pathlib import Path


def main(dst):
    here = Path(__file__).resolve().parent
    sys.path.insert(0, str(Path.cwd()))
    import mile_amd
    print('library side:', Path(mile_amd.__file__).resolve().parent)
    spec = importlib.util.spec_from_file_location('w64_edges', here.parent / 'test_gpu_w64_edges.py')
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    out = {}
    for form in T.FORMS:
        for N in T.CASES:
            info, lp, g = T.run(form, N)
            out[T.key_of(form, N)] = T.digest(lp[:2], g[:2])
            print(T.key_of(form, N), info['grid'], out[T.key_of(form, N)][:16], flush=True)
    Path(dst).write_text(json.dumps(out, indent=1, sort_keys=True) + '\n')
    print('wrote', dst, len(out))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'w64_edges_parent.json')
