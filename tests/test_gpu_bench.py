"""bench.py --dump-outputs: the outputs of the last timed step are written, and two runs with the same arguments compute the
same thing from the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--image', '32',
           '--ngeo', '32', '--frames', '8', '--frames-per-gpu', '4', '--width', '64', '--no-cpu-baseline', '--no-parity-mode',
           '--no-tutorial-domain', '--dump-outputs', str(out_dir)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=540)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return json.loads([l for l in res.stdout.splitlines() if l.startswith('{"metric"')][-1])


@pytest.mark.timeout(600)
def test_dump_outputs_of_the_last_timed_step(tmp_path):
    r1 = _bench(tmp_path / 'a', 3)
    assert r1['steps'] == 3 and r1['ms_per_step'] > 0
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['adam_m.npy', 'adam_v.npy', 'images.npy', 'loss.npy', 'params.npy']
    out = {n[:-4]: np.load(tmp_path / 'a' / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out['images'].size == 4 * 32 * 32 and np.abs(out['images']).max() > 0
    assert out['params'].shape == out['adam_m'].shape == out['adam_v'].shape and np.abs(out['adam_m']).max() > 0
    # the same arguments: the same inputs, so the same outputs (the step is deterministic, tests/test_gpu_fullsize.py)
    _bench(tmp_path / 'b', 3)
    for n in names:
        assert np.array_equal(out[n[:-4]], np.load(tmp_path / 'b' / n)), n
    # --steps sets the number of timed steps: one more step moves the parameters again
    r3 = _bench(tmp_path / 'c', 4)
    assert r3['steps'] == 4 and not np.array_equal(out['params'], np.load(tmp_path / 'c' / 'params.npy'))
