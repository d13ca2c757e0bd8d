"""bench.py contract checks: the multi-GPU launcher logic and the --dump-outputs sample (CPU); on the GPU box the plain line,
the --full line and the RCCL code path with one rank."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=900):
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    env.pop('RANK', None)
    env.pop('LOCAL_RANK', None)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_gpus_n_without_enough_devices_fails_loudly():
    """`python bench.py --gpus N` (how the driver starts it) must never run a smaller job under the label n_gpus=N."""
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    r = _run(['--gpus', str(have + 2), '--steps', '1', '--warmup', '0'], timeout=300)
    assert r.returncode != 0
    assert f'only {have} GPU(s) visible' in (r.stderr + r.stdout)


def test_dump_outputs_keeps_a_seeded_sample_under_the_budget(tmp_path):
    """--dump-outputs: whole arrays when they fit; above the byte budget the same seeded sample of whole images on every call,
    with the indices it kept."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    a = np.random.default_rng(5).standard_normal((40, 3, 16, 16)).astype(np.float64)
    bench.dump_outputs(str(tmp_path / 'all'), {'images': a}, budget=1 << 20)
    whole = np.load(tmp_path / 'all' / 'images.npy')
    assert whole.dtype == np.float32 and np.array_equal(whole, a.astype(np.float32))
    assert not (tmp_path / 'all' / 'images_index.npy').exists()
    for d in ('s1', 's2'):
        bench.dump_outputs(str(tmp_path / d), {'images': a}, budget=40_000)
    s, idx = np.load(tmp_path / 's1' / 'images.npy'), np.load(tmp_path / 's1' / 'images_index.npy')
    assert idx.dtype == np.float64 and 0 < len(idx) < len(a) and np.array_equal(s, whole[idx.astype(np.int64)])
    assert np.array_equal(s, np.load(tmp_path / 's2' / 'images.npy'))
    assert sum(f.stat().st_size for f in (tmp_path / 's1').iterdir()) <= 40_000


@pytest.mark.gpu
def test_plain_line_times_the_headline_only_and_dumps_its_images(tmp_path):
    """A plain run: the headline leg only, exactly --steps timed steps, and --dump-outputs writes the images of the last timed
    step -- the generator's output on the seeded benchmark inputs (oracle, 1e-3 like every parity test)."""
    import numpy as np
    B, S, ngf = 2, 128, 16
    r = _run(['--steps', '3', '--warmup', '1', '--batch', str(B), '--size', str(S), '--ngf', str(ngf), '--dump-outputs', str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 3 and line['step_ms']['n'] == 3 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'images/s' and line['higher_is_better'] is True and line['dtype'].startswith('f32 (every product')
    for k in ('f32_class_f16x3', 'face_like_labels', 'pipeline', 'roofline', 'cpu_baseline', 'interactive_b1', 'host_enqueue_ms_per_step'):
        assert k not in line, k
    img = np.load(tmp_path / 'images.npy')
    assert img.dtype == np.float32 and img.shape == (B, 3, S, S)
    from ctrlhair_amd import procedural as P
    from oracle import sean_oracle as O
    ref = O.generator_forward(O.to_torch(P.sean_state_dict(0, ngf)), P.blocky_labels(B, S), P.style_codes(B),
                              P.noise_planes(B, S, ngf), ngf).numpy()
    assert float(np.abs(img - ref).max()) <= 1e-3


@pytest.mark.gpu
def test_force_dist_runs_the_rccl_path_on_one_gpu():
    """1-rank NCCL (= RCCL) process group: PipelinedGather's all_gather_into_tensor on a side stream, slot check, JSON line."""
    r = _run(['--full', '--force-dist', '--only-headline', '--no-cpu-baseline', '--steps', '3', '--warmup', '1', '--batch', '2', '--size', '256'])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['n_gpus'] == 1 and line['value'] > 0 and 'RCCL all-gather' in line['config']['parallelism']
    assert line['dtype'].startswith('f32 (every product and sum an IEEE f32') and line['step_ms']['n'] == 3
    rf = line['roofline']
    assert rf['bound'] == 'mfma' and 0 < rf['frac'] < 1 and rf['flops_executed_per_launch_avg'] <= rf['flops_dense_per_launch_avg'] * 1.001


@pytest.mark.gpu
def test_default_line_carries_every_block():
    """The --full line: exact-f32 top level + f16x3 block + face-like labels + Config 3 pipeline (small sizes here)."""
    r = _run(['--full', '--no-cpu-baseline', '--steps', '3', '--warmup', '1', '--batch', '2', '--size', '256'])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'f32_class_f16x3', 'face_like_labels', 'pipeline', 'sustained_peaks'):
        assert k in line, k
    assert line['config']['conv_path'] == 'f32' and line['f32_class_f16x3']['value'] > 0
    assert set(line['pipeline']) >= {'f16x3', 'f32'} and 'stages' in line['pipeline']['f16x3']
    assert line['face_like_labels']['f32']['value'] > 0
    assert line['host_enqueue_ms_per_step']['n'] == 3 and line['host_enqueue_ms_per_step']['median'] > 0
    for leg in ('f16x3', 'f32'):         # stage rows: executed FLOPs against the peak of the unit that ran them -- never above it
        for name, row in line['pipeline'][leg]['stages'].items():
            if row.get('bound') == 'mfma':
                assert 0 <= row['frac'] < 1 and 0 < row['executed_tflops'] <= row['peak_tflops'], (leg, name, row)      # (tiny here: 2 x 256^2)
