"""bench.py's contract: a plain run times exactly --steps steps and carries nothing of --full; --dump-outputs writes the loss and
the trained variables of the last step as float32 / float64 .npy files, the same ones for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


class _FakeEngine(object):
    """The slice of HipEngine dump_outputs reads, on host tensors."""

    def __init__(self, M=1000, K=8, D=4):
        g = torch.Generator().manual_seed(3)
        self.inner = torch.randn((M, K), generator=g)
        self.outer = torch.randn((M, D), generator=g)
        self.fbias = torch.randn((M,), generator=g)

    def export_params_dense(self):
        return {'bias': np.float32(0.25), 'dense_kernel': np.arange(6, dtype=np.float32).reshape(6, 1)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_whole_small_tables(tmp_path):
    import bench
    eng = _FakeEngine()
    bench.dump_outputs(str(tmp_path), eng, 0.5)
    got = _load(str(tmp_path))
    assert set(got) == {'loss', 'bias', 'dense_kernel', 'inner_embeddings', 'outer_embeddings', 'feature_bias'}
    assert got['loss'].dtype == np.float64 and got['loss'].tolist() == [0.5]
    assert all(v.dtype == np.float32 for k, v in got.items() if k != 'loss')
    assert np.array_equal(got['inner_embeddings'], eng.inner.numpy())
    assert np.array_equal(got['feature_bias'], eng.fbias.numpy().reshape(-1, 1))


def test_dump_outputs_samples_large_tables_the_same_way_every_time(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_TABLE_BYTES', 4 * 13 * 100)         # 100 rows of K + D + 1 = 13 floats
    eng = _FakeEngine()
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    bench.dump_outputs(a, eng, 1.0)
    bench.dump_outputs(b, eng, 1.0)
    da, db = _load(a), _load(b)
    rows = da['table_rows']
    assert rows.dtype == np.float64 and rows.shape == (100,)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 1000
    r = rows.astype(np.int64)
    assert np.array_equal(da['outer_embeddings'], eng.outer.numpy()[r])
    assert set(da) == set(db) and all(np.array_equal(da[k], db[k]) for k in da)


@pytest.mark.gpu
def test_plain_bench_times_exactly_the_steps_and_dumps(tmp_path):
    out = str(tmp_path / 'dump')
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '2',
                        '--dump-outputs', out], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    assert res['steps'] == 7 and res['blocks'] == 1 and len(res['ms_per_step_blocks']) == 1
    assert res['ms_per_step'] > 0 and res['value'] > 0 and res['unit'] == 'examples/s' and res['higher_is_better'] is True
    for k in ('roofline', 'stress', 'stage_us', 'cpu_baseline', 'value_with_host_batching'):
        assert k not in res, k
    got = _load(out)
    assert got['loss'].dtype == np.float64 and np.isclose(got['loss'][0], res['final_loss'], rtol=1e-5, atol=1e-6)
    assert got['inner_embeddings'].shape == (5382, 32) and got['feature_bias'].shape == (5382, 1)
    assert all(np.isfinite(v).all() and v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 << 20
