"""A plain `python bench.py --gpus 1 --steps K --warmup W` does only what its headline needs: set-up, warm-up, the timed steps,
--dump-outputs and the JSON line.  The rooflines, the CPU baseline and parity, the secondary configs and the training update
belong to `--full`; a plain run spends at most 30 s outside its steps."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ('roofline', 'roofline_conv', 'cpu_baseline', 'parity', 'secondary', 'train_step', 'train_step_dp')


def test_a_plain_run_prints_the_headline_alone_within_its_budget(tmp_path):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR'):
        env.pop(k, None)
    steps, warmup = 3, 1
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                        '--dump-outputs', str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line['metric'] == 'inpainted frames/sec (128x128, K=F=5, T=5)' and line['unit'] == 'frames/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['steps'] == steps and line['warmup'] == warmup
    # value = frames of the timed steps / their time, ms_per_step = that time / steps (each rounded in the line)
    assert line['value'] > 0 and abs(line['value'] * line['ms_per_step'] / 1e3 / (32 * 5) - 1) < 1e-3
    assert not [k for k in FULL_ONLY if k in line], sorted(line)
    arrays = line['dumped_outputs']['arrays']
    assert arrays and sorted(f[:-4] for f in os.listdir(tmp_path)) == sorted(arrays)
    assert all(np.isfinite(np.load(tmp_path / (k + '.npy'))).all() for k in arrays)
    outside = wall - (steps + warmup) * line['ms_per_step'] / 1e3
    assert outside < 30.0, 'a plain run spent %.1f s outside its steps' % outside
