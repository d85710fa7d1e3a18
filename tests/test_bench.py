"""bench.py: the driver contract (one JSON line on stdout, the keys the driver reads; `roofline` / `cpu_baseline`
objects with --full), --dump-outputs, and the multi-rank launcher's refusals."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=600):
    e = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=timeout)


def test_bare_multi_gpu_launch_refuses_without_enough_gpus():
    """`python bench.py --gpus N` without WORLD_SIZE becomes the launcher (torch.distributed.run children, as
    tools/dist_train.sh:9-18); on a box with fewer than N GPUs it must fail loudly, never run N = 1 silently"""
    import torch
    if torch.cuda.device_count() >= 8:
        pytest.skip('box has 8 GPUs')
    r = _run(['--gpus', '8', '--steps', '1', '--warmup', '0'], timeout=120)
    assert r.returncode != 0
    assert r.stdout.strip() == '' and 'GPU' in r.stderr


def test_world_size_mismatch_is_an_error():
    r = _run(['--gpus', '2', '--steps', '1', '--warmup', '0'], env={'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0'},
             timeout=120)
    assert r.returncode != 0 and 'WORLD_SIZE' in r.stderr and r.stdout.strip() == ''


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['train', 'infer'])
def test_bench_prints_one_json_line_with_the_contract_keys(mode):
    r = _run(['--steps', '3', '--warmup', '1', '--mode', mode, '--cpu-baseline-seconds', '2', '--full'], timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:1000]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1 and d['value'] > 0 and d['ms_per_step'] > 0
    assert d['unit'] == 'images/s' and d['higher_is_better'] is True and d['scaling'] == 'weak'
    assert d['vs_baseline'] is None and d['dtype'] == 'bf16' and d['data'] == 'synthetic'
    assert '1024x1024' in d['metric'] and 'workload' in d['config'] and 'model' not in d['config']
    assert abs(d['value'] - d['config']['global_batch'] / (d['ms_per_step'] * 1e-3)) < 0.02 * d['value']
    rf = d['roofline']
    assert rf['bound'] in ('hbm', 'mfma') and rf['unit'] in ('GB/s', 'TFLOP/s') and 0 < rf['frac'] < 1
    assert abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-3 and 'traffic' in rf and rf['kernel']
    cb = d['cpu_baseline']
    assert cb['kind'] == 'port' and cb['value'] > 0 and cb['cores'] >= 1 and cb['sample']


def test_steps_must_be_positive():
    r = _run(['--steps', '0', '--warmup', '0'], timeout=120)
    assert r.returncode != 0 and '--steps' in r.stderr and r.stdout.strip() == ''


def test_dump_outputs_stays_within_budget_and_samples_the_same_positions(tmp_path, monkeypatch):
    """arrays that do not fit are replaced by the same seeded sample of their elements in every run, drawn from a
    generator of its own (the process's global random stream is left as it was).  A small budget stands in for the
    64 MB one: same code path, no large allocations in the test process."""
    import numpy as np
    import torch
    monkeypatch.syspath_prepend(ROOT)
    import bench
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 6000)
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(2, 2, 16, 32, generator=g)
    mask = torch.randint(0, 2, (2, 16, 32), dtype=torch.uint8, generator=g)
    rng = torch.get_rng_state()
    runs = []
    for d in ('a', 'b'):
        bench.dump_outputs(bench.step_outputs('infer', (logits, mask), None), str(tmp_path / d))
        runs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    assert torch.equal(torch.get_rng_state(), rng)
    assert sorted(runs[0]) == ['pred_sem_seg.npy', 'seg_logits.npy']
    for f, a in runs[0].items():
        assert a.dtype == np.float32 and a.size == 6000 // 2 // 4 and np.array_equal(a, runs[1][f])
    assert sum(a.nbytes for a in runs[0].values()) <= 6000
    assert np.isin(runs[0]['seg_logits.npy'], logits.numpy()).all()
    small = {'decode.loss_context': torch.tensor(1.5), 'parameters': torch.arange(10, dtype=torch.float64)}
    bench.dump_outputs(small, str(tmp_path / 'c'))
    assert np.load(tmp_path / 'c' / 'decode.loss_context.npy') == np.float32(1.5)
    p = np.load(tmp_path / 'c' / 'parameters.npy')
    assert p.dtype == np.float64 and np.array_equal(p, np.arange(10))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['train', 'infer'])
def test_plain_bench_times_the_steps_and_dumps_reproducible_outputs(mode, tmp_path):
    """a plain run prints the contract keys without the --full measurements; --dump-outputs writes the same outputs in
    every run, whatever the number of steps timed before: inference the last timed step (no state), training one step
    of the timed path from the run's start state.  Bounds relative to each array's largest magnitude: training 1e-2
    (bf16 activations, atomics-ordered sums: two runs measured 1.1e-3 in the parameters, 2e-4 in the loss), inference
    1e-5 (measured bit-identical)."""
    import numpy as np
    dumps = []
    for steps, warmup in ((2, 1), (3, 2)):
        out = tmp_path / f'out{steps}'
        r = _run(['--steps', str(steps), '--warmup', str(warmup), '--mode', mode, '--dump-outputs', str(out)], timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout[:1000]
        d = json.loads(lines[0])
        assert d['steps'] == steps and d['warmup'] == warmup and d['ms_per_step'] > 0 and d['value'] > 0
        assert d['unit'] == 'images/s' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
        assert abs(d['value'] - d['config']['global_batch'] / (d['ms_per_step'] * 1e-3)) < 0.02 * d['value']
        assert not {'roofline', 'cpu_baseline', 'parity', 'deterministic_mode'} & set(d)
        files = sorted(os.listdir(out))
        assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10 ** 6
        arrays = {f[:-4]: np.load(out / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        if mode == 'train':
            assert {'decode.loss_context', 'decode.loss_spatial', 'parameters', 'buffers'} <= set(arrays)
            assert arrays['decode.loss_context'] > 0
        else:
            assert set(arrays) == {'seg_logits', 'pred_sem_seg'}
            assert set(np.unique(arrays['pred_sem_seg'])) <= {0.0, 1.0}
        dumps.append(arrays)
    assert sorted(dumps[0]) == sorted(dumps[1])
    tol = 1e-2 if mode == 'train' else 1e-5
    for k, a in dumps[0].items():
        b = dumps[1][k].astype(np.float64)
        a = a.astype(np.float64)
        assert np.abs(a - b).max() <= tol * max(np.abs(a).max(), 1e-30), (k, np.abs(a - b).max(), np.abs(a).max())
