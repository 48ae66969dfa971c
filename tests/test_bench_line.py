"""
bench.py's N > 1 line explains itself: a same-device rehearsal of two ranks on the one GPU of the test
box, started as a child process exactly as a user would (`python bench.py --gpus 2 ...` spawns its ranks through
torch.distributed.run before touching the GPU), must name the exchange it ran, why, every rank's device, and the step
time through each exchange.  One device: `--steps` is the number of timed steps, and `--dump-outputs` repeats bitwise.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_rank_same_device_bench_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--same-device', '--backend', 'gloo',
                        '--steps', '5', '--warmup', '2'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{') and '"metric"' in ln]
    assert len(lines) == 1
    d = json.loads(lines[0])
    c = d['config']
    assert d['n_gpus'] == 2 and c['world_size'] == 2 and c['same_device_rehearsal'] is True
    assert c["dp_exchange"].startswith("peer-mapped buffers"), c
    assert "calibrated on this step" in c["dp_exchange_reason"]
    assert 'self-check passed' in c['dp_exchange_reason']
    assert [v['rank'] for v in c['devices']] == [0, 1] and all(v['name'] for v in c['devices'])
    by = c['ms_per_step_by_exchange']
    assert len(by) >= 4 and all(v > 0 for v in by.values())
    assert any(k.startswith('all_reduce (gloo)') for k in by) and any(k.startswith('separate one-workgroup') for k in by)
    assert d['value'] > 0 and d['ms_per_step'] > 0 and d['scaling'] == 'weak'


def test_dump_outputs_repeat_bitwise_and_belong_to_the_last_timed_step(tmp_path):
    """--steps K times exactly K steps and --dump-outputs writes the last one's parameters, gradients and [sse, sum y^2]
    as float64 .npy files, bitwise the same in a second run with the same arguments.  The timed steps cycle the 32
    resident batches from batch 0, so the dumped sum y^2 is that of batch (K - 1) mod 32 of bench.synth."""
    import importlib.util
    import numpy as np
    steps = 37
    dumps = []
    for run in range(2):
        out = tmp_path / f'run{run}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '3',
                            '--no-cpu-baseline', '--no-secondary', '--budget-scale', '0.05', '--dump-outputs', str(out)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{') and '"metric"' in ln][-1])
        assert d['steps'] == steps and d['timing']['timed_steps'] == steps and d['ms_per_step'] > 0
        dumps.append({n: np.load(out / f'{n}.npy') for n in ('params', 'grads', 'loss_sums')})
    for n, a in dumps[0].items():
        assert a.dtype == np.float64 and np.isfinite(a).all(), n
        assert a.shape == dumps[1][n].shape and a.tobytes() == dumps[1][n].tobytes(), n
    assert dumps[0]['params'].shape == dumps[0]['grads'].shape == (2401,) and dumps[0]['loss_sums'].shape == (2,)
    spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    _, _, y = bench.synth(0, 32 * bench.BATCH)
    b = (steps - 1) % 32
    want = float((y[b * bench.BATCH:(b + 1) * bench.BATCH] ** 2).sum())
    assert abs(dumps[0]['loss_sums'][1] - want) <= 1e-12 * want
    assert dumps[0]['loss_sums'][0] > 0
