"""Writes the digests tests/test_gpu_step_edges.py compares with (step_edges_parent.json), from whatever build is imported.

The committed file was written by this script on an MI355X from a checkout of the commit BEFORE the small-accumulator phase of
k_grad_w64's reduction was shortened (`git log -- mile_amd/csrc/mile_grad_w64.h`, the commit that added this file), with that
commit's library:

    git worktree add ../before <that commit> && (cd ../before && python __graft_entry__.py)
    cd ../before && python <this checkout>/tests/golden/make_step_edges_digests.py out.json

It takes mile_amd and the oracle from the current directory and the cases, the runs and the digest from the test module next
to it, so the reference side and the tested side run the same inputs through the same code.  Regenerate only from a build whose
steps are known good: the digests are the reference, not a property of the inputs.
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
    spec = importlib.util.spec_from_file_location('step_edges', here.parent / 'test_gpu_step_edges.py')
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    out = {}
    for case in T.CASES:
        for name, calls in T.RUNS.items():
            key = f'{T.case_id(case)}-steps{name}'
            out[key] = T.digest(T.run_steps(case, calls))
            print(key, out[key][:16], flush=True)
    key = f'{T.case_id(T.TUNE_CASE)}-tune3'
    out[key] = T.digest(T.run_tune(T.TUNE_CASE))
    print(key, out[key][:16], flush=True)
    Path(dst).write_text(json.dumps(out, indent=1, sort_keys=True) + '\n')
    print('wrote', dst, len(out))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'step_edges_parent.json')
