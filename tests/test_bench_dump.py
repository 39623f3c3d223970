"""bench.py --dump-outputs (bench.dump_outputs) on host tensors: the files a run leaves,
their shapes and dtype, the untiling, and the fixed seeded sample of a batch whose
arrays would exceed the byte budget."""
import os

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

import bench
from apf_quadruped_amd import plans
from apf_quadruped_amd.batch import Plan, to_tiled

NAMES = {"x": 12, "y": 6, "z": 20, "s": 20, "stats": 6}


@pytest.fixture(scope="module")
def filled():
    """The C1 plan and host outputs of a 200-QP batch (four tiles, the last one partial)
    holding known per-QP rows."""
    import torch
    B = 200
    d0 = plans.standard_qp("c1")
    plan = Plan.from_dense(12, 20, 6, d0["P"][0], d0["A"][0], d0["G"][0])
    rng = np.random.default_rng(5)
    rows = {k: rng.standard_normal((B, w)) for k, w in NAMES.items()}
    rows.update(fval=rng.standard_normal(B), flag=rng.integers(0, 3, B), iters=rng.integers(1, 100, B))
    out = plan.alloc_outputs(B, device="cpu")
    for k in NAMES:
        out[k].zero_()
        out[k][:to_tiled(rows[k]).size] = torch.from_numpy(to_tiled(rows[k]))
    for k in ("fval", "flag", "iters"):
        out[k].copy_(torch.from_numpy(rows[k]))
    return plan, B, out, rows, torch.tensor([-3.5, 17.0], dtype=torch.float64)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_whole_batch(filled, tmp_path):
    plan, B, out, rows, best = filled
    bench.dump_outputs(str(tmp_path / "d"), plan, B, out, best, None, 0)
    got = _load(tmp_path / "d")
    assert set(got) == set(NAMES) | {"fval", "flag", "iters", "best"}
    assert all(a.dtype == np.float64 for a in got.values())
    for k in rows:
        assert np.array_equal(got[k], rows[k]), k
    assert got["best"].tolist() == [-3.5, 17.0]


def test_dump_outputs_samples_past_the_budget(filled, tmp_path):
    plan, B, out, rows, best = filled
    budget = 20_000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), plan, B, out, best, None, 0, budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    ids = a["rows"].astype(np.int64)
    assert 0 < len(ids) < B and np.all(np.diff(ids) > 0) and ids[-1] < B
    assert sum(v.nbytes for v in a.values()) <= budget
    for k in rows:
        assert np.array_equal(a[k], rows[k][ids]), k
    assert all(np.array_equal(a[k], b[k]) for k in a)      # the same sample every run


def test_dump_outputs_rank_suffix(filled, tmp_path):
    plan, B, out, rows, best = filled
    import torch
    bench.dump_outputs(str(tmp_path), plan, B, out, best, torch.arange(14, dtype=torch.float64), 1)
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".rank1.npy" for k in
                                                  list(NAMES) + ["fval", "flag", "iters", "best", "winner"])
