"""bench.py's command line: the plain run's one result line and ``--dump-outputs``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(tmp_path):
    d = str(tmp_path / 'dump')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps',
                        '3', '--warmup', '1', '--dump-outputs', d],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1                       # stdout carries the result line and nothing else
    out = json.loads(lines[0])
    assert out['steps'] == 3 and out['warmup'] == 1
    assert out['unit'] == 'trained images/s' and out['higher_is_better'] is True
    assert out['dtype'] == 'bf16' and out['ms_per_step'] > 0
    # value and ms_per_step are the same measurement: batch 32 on one GPU
    assert abs(out['value'] - 32e3 / out['ms_per_step']) <= 1e-3 * out['value']
    # what --full measures stays out of a plain run
    assert out['sampler_overhead_pct'] is None
    assert not {'device_phase_ms', 'dp', 'solo_ms'} & set(out)
    files = sorted(os.listdir(d))
    assert files == ['bn_running_mean.npy', 'bn_running_var.npy', 'pool_losses.npy',
                     'pool_mean_ema.npy']
    total = 0
    for f in files:
        a = np.load(os.path.join(d, f))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    losses = np.load(os.path.join(d, 'pool_losses.npy'))
    assert losses.shape == (320,) and (losses > 0).all()
    assert np.load(os.path.join(d, 'bn_running_mean.npy')).size == 4800   # ResNet-18's BN channels
    # the last timed step starts from the seeded initial state: at random init the losses sit
    # near ln(10), and the pool mean is the mean of the dumped pool (fp32 sum of 320 values)
    pool_mean, ema = np.load(os.path.join(d, 'pool_mean_ema.npy'))
    assert 1.5 < pool_mean < 4.0 and 1.5 < ema < 4.0
    assert abs(losses.mean() - pool_mean) < 1e-4 * pool_mean
    assert out['final_train_loss'] > 0
