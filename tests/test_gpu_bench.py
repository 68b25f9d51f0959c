"""bench.py end to end on the GPU (-m gpu): a plain run prints the headline line and nothing it does not need;
--full adds the roofline pass and the CPU baseline to the same line."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = Path(__file__).resolve().parents[1]


def _bench(*extra, timeout=300):
    r = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5', *extra],
                       capture_output=True, text=True, timeout=timeout, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _check_headline(out):
    assert out['metric'].startswith('MCLMC integrator particle-steps/s') and out['unit'] == 'particle-steps/s'
    assert out['higher_is_better'] is True and out['dtype'] == 'f32' and (out['steps'], out['warmup']) == (20, 5)
    assert out['ms_per_step'] > 0 and out['value'] > 0 and out['config']['finite']
    assert out['value'] == pytest.approx(out['config']['ensemble_per_gpu'] / (out['ms_per_step'] * 1e-3), rel=1e-3)


def test_plain_run_is_the_headline_only():
    out = _bench()
    _check_headline(out)
    assert out['roofline'] is None and out['cpu_baseline'] is None and 'secondary' not in out


def test_full_run_adds_roofline_and_cpu_baseline():
    out = _bench('--full', '--no-secondary')
    _check_headline(out)
    assert out['roofline']['launches_timed'] > 0 and out['roofline']['achieved'] > 0
    assert out['cpu_baseline']['value'] > 0 and 'secondary' not in out
