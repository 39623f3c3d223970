"""On-device assembly of the controller's trot and crawl QPs (qpb_assemble_gait)
against its numpy restatement workloads.controller_gait_qp_from_terms
(main.cpp:1730-2005, :2486-2695, :2915-3232).

Copies, signs and constants (identity, +-1, +-mu, slack weights, Mcom, +-Mjj, +-Jst
entries, the negated b terms) are bit-exact.  The computed entries -- the force block
of P, c and h -- stay within 1e-14 * max(1, largest computed |entry| of the array):
the bar of the stance test (tests/test_controller_assemble.py), the slack weight kept
out of the scale.  The assembled values then reach the solver: at tol 1e-6 the
solutions are the oracle's within the project's north-star bar 1e-6 * max(1, |x|_inf)
(QP_OPTIMAL for every case: tests/test_gait_assemble.py)."""
import functools

import numpy as np
import pytest

from apf_quadruped_amd import workloads as W

SEED = 0xD06B07 + 61
TROT, CRAWL = (0xA, 0x5), (0xE, 0xB, 0xD, 0x7)
CASES = [(s, f) for s in TROT for f in (False, True)] + [(s, False) for s in CRAWL]


@functools.lru_cache(maxsize=None)
def _terms(stance, B=200):
    t = W.controller_gait_terms(SEED, np.arange(B), stance)
    for v in t.values():
        v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _ref(stance, dyn, B=200):
    d = W.controller_gait_qp_from_terms(_terms(stance, B), stance, trot_b_dynamics=dyn)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _plan_of(d):
    from apf_quadruped_amd.batch import Plan
    return Plan.from_dense(30, d["m"], d["p"], d["P"][0], d["A"][0], d["G"][0])


def _dense_from_tiled(plan, out, B):
    """Tiled CSC values -> dense [B, r, c] with the plan's patterns (P upper mirrored)."""
    from apf_quadruped_amd.batch import from_tiled
    res = {}
    for k, (jc, ir), shape in (("P", plan.patterns.P, (30, 30)), ("A", plan.patterns.A, (plan.p, 30)),
                               ("G", plan.patterns.G, (plan.m, 30))):
        v = from_tiled(out[k], B, len(ir)).cpu().numpy()
        M = np.zeros((B,) + shape)
        cols = np.repeat(np.arange(len(jc) - 1), np.diff(jc))
        M[:, ir, cols] = v
        if k == "P":
            M = M + np.transpose(M, (0, 2, 1)) - M * np.eye(30)[None]
        res[k] = M
    for k, nv in (("c", 30), ("h", plan.m), ("b", plan.p)):
        res[k] = from_tiled(out[k], B, nv).cpu().numpy()
    return res


def _device_inputs(t):
    import torch
    from apf_quadruped_amd.batch import to_tiled
    return (torch.from_numpy(to_tiled(W.pack_terms(t))).cuda(), torch.from_numpy(to_tiled(W.pack_swing(t))).cuda())


def _check_values(got, ref, stance):
    """got / ref dense dicts of the same QPs: exact where copied, 1e-14 where computed."""
    o_s = 18 + 3 * bin(stance).count("1")
    for k in ("A", "G", "b"):
        assert np.array_equal(got[k], ref[k]), k
    force = np.zeros((30, 30), bool)
    force[18:o_s, 18:o_s] = True
    assert np.array_equal(got["P"][:, ~force], ref["P"][:, ~force])
    assert np.array_equal(got["c"][:, :18], ref["c"][:, :18]) and np.array_equal(got["c"][:, o_s:], ref["c"][:, o_s:])
    worst = {}
    for k, sel in (("P", (slice(None), force)), ("c", (slice(None), slice(18, o_s))), ("h", (slice(None),))):
        scale = max(1.0, float(np.abs(ref[k][sel]).max()))
        worst[k] = float(np.abs(got[k][sel] - ref[k][sel]).max()) / scale
        print(f"mask {stance:#x} {k}: max deviation {worst[k]:.3e} of scale {scale:.6g}")
    for k, w in worst.items():
        assert w <= 1e-14, (k, w)


@pytest.mark.gpu
@pytest.mark.parametrize("stance,dyn", CASES)
def test_assemble_gait_matches_restatement_and_solves(stance, dyn, oracle):
    import torch
    B = 200                                         # three full tiles and a partial one
    t, ref = _terms(stance), _ref(stance, dyn)
    plan = _plan_of(ref)
    terms, swing = _device_inputs(t)
    chk = torch.zeros(B, dtype=torch.int32, device="cuda")
    vals = plan.assemble_gait(terms, stance, swing=swing, B=B, trot_b_dynamics=dyn, check=chk)
    torch.cuda.synchronize()
    assert (chk.cpu().numpy() == 1).all()
    _check_values(_dense_from_tiled(plan, vals, B), ref, stance)
    r = plan.unpack(plan.solve(**vals, B=B, reltol=1e-6, abstol=1e-6), B)
    Pc, Ac, Gc = W.to_colmajor(ref["P"]), W.to_colmajor(ref["A"]), W.to_colmajor(ref["G"])
    worst = 0.0
    for q in range(0, B, 23):
        o = oracle.solve_dense(30, ref["m"], ref["p"], Pc[q], Ac[q], Gc[q], ref["c"][q], ref["h"][q], ref["b"][q],
                               perm=plan.perm, reltol=1e-6, abstol=1e-6)
        assert r["flag"][q] == 0 and o["flag"] == 0, (q, r["flag"][q], o["flag"])
        worst = max(worst, float(np.abs(r["x"][q] - o["x"]).max()) / max(1.0, float(np.abs(o["x"]).max())))
    print(f"mask {stance:#x} trot_b_dynamics={dyn}: max |x - oracle| / max(1, |x|_inf) = {worst:.3e}")
    assert worst <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("stance", [0x5, 0xB])
def test_assemble_gait_shared_terms(stance):
    """One shared copy of terms and swing plus a per-candidate tiled wdes: bit-identical
    to the tiled call on the replicated terms."""
    import torch
    from apf_quadruped_amd.batch import from_tiled, to_tiled
    B = 65
    one = {k: v[:1] for k, v in _terms(stance).items()}
    wd = _terms(stance)["wdes"][:B]
    plan = _plan_of(_ref(stance, False))
    chk = torch.zeros(B, dtype=torch.int32, device="cuda")
    shared = plan.assemble_gait(torch.from_numpy(W.pack_terms(one)[0].copy()).cuda(), stance,
                                swing=torch.from_numpy(W.pack_swing(one)[0].copy()).cuda(), B=B, shared=True,
                                swing_shared=True, wdes=torch.from_numpy(to_tiled(wd)).cuda(), check=chk)
    rep = {k: np.repeat(v, B, 0) for k, v in one.items()}
    rep["wdes"] = wd
    terms, swing = _device_inputs(rep)
    tiled = plan.assemble_gait(terms, stance, swing=swing, B=B)
    torch.cuda.synchronize()
    assert (chk.cpu().numpy() == 1).all()
    for k, nv in (("P", plan.info.nnzP), ("A", plan.info.nnzA), ("G", plan.info.nnzG), ("c", 30), ("h", plan.m),
                  ("b", plan.p)):
        assert torch.equal(from_tiled(shared[k], B, nv), from_tiled(tiled[k], B, nv)), k
    _check_values(_dense_from_tiled(plan, shared, B), W.controller_gait_qp_from_terms(rep, stance), stance)


@pytest.mark.gpu
def test_assemble_gait_stance_mask_is_assemble_controller():
    import torch
    from apf_quadruped_amd.batch import Plan, from_tiled
    B = 65
    t = {k: v[:B] for k, v in _terms(0xF).items()}
    d = W.controller_qp_from_terms(t)
    plan = Plan.from_dense(30, 68, 18, d["P"][0], d["A"][0], d["G"][0], order="amd")
    terms, swing = _device_inputs(t)
    chk = [torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3)]
    want = plan.assemble_controller(terms, B=B, check=chk[0])
    got = plan.assemble_gait(terms, 0xF, B=B, check=chk[1])                       # swing may be absent
    got2 = plan.assemble_gait(terms, 0xF, swing=swing, B=B, trot_b_dynamics=True, check=chk[2])
    torch.cuda.synchronize()
    for k, nv in (("P", plan.info.nnzP), ("A", plan.info.nnzA), ("G", plan.info.nnzG), ("c", 30), ("h", 68), ("b", 18)):
        assert torch.equal(from_tiled(got[k], B, nv), from_tiled(want[k], B, nv)), k
        assert torch.equal(from_tiled(got2[k], B, nv), from_tiled(want[k], B, nv)), k
    assert all((c.cpu().numpy() == 1).all() for c in chk)


@pytest.mark.gpu
@pytest.mark.parametrize("stance", [0xA, 0xE])
def test_assemble_gait_flags_off_pattern_terms(stance):
    import torch
    B = 64
    t = {k: v[:B].copy() for k, v in _terms(stance).items()}
    t["Jst"][:, 0, 9] = 0.0            # swing foot BR, row x, a joint of another leg: an exact zero ...
    plan = _plan_of(W.controller_gait_qp_from_terms(t, stance))
    t["Jst"][5, 0, 9] = 1e-3           # ... which QP 5 violates
    terms, swing = _device_inputs(t)
    chk = torch.zeros(B, dtype=torch.int32, device="cuda")
    plan.assemble_gait(terms, stance, swing=swing, B=B, check=chk)
    c = chk.cpu().numpy()
    assert c[5] == 0 and (np.delete(c, 5) == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("stance", [0x5, 0x7])
def test_assemble_gait_edges(stance):
    """B = 1, and B = 65 into sentinel-filled buffers: lanes 1..63 of the second tile
    are not written."""
    import torch
    plan = _plan_of(_ref(stance, False))
    sentinel = -12345.678
    for B in (1, 65):
        t = {k: v[:B] for k, v in _terms(stance).items()}
        T = 64 * ((B + 63) // 64)
        sizes = dict(P=plan.info.nnzP, A=plan.info.nnzA, G=plan.info.nnzG, c=30, h=plan.m, b=plan.p)
        out = {k: torch.full((nv * T,), sentinel, dtype=torch.float64, device="cuda") for k, nv in sizes.items()}
        chk = torch.full((T,), 7, dtype=torch.int32, device="cuda")
        terms, swing = _device_inputs(t)
        got = plan.assemble_gait(terms, stance, swing=swing, B=B, out=out, check=chk)
        torch.cuda.synchronize()
        assert got is out
        _check_values(_dense_from_tiled(plan, out, B), W.controller_gait_qp_from_terms(t, stance), stance)
        c = chk.cpu().numpy()
        assert (c[:B] == 1).all() and (c[B:] == 7).all()
        for k, nv in sizes.items():
            last = out[k].reshape(T // 64, nv, 64)[-1].cpu().numpy()        # [slot, lane] of the last tile
            lanes = (B - 1) % 64 + 1
            assert (last[:, lanes:] == sentinel).all(), k
            assert (last[:, :lanes] != sentinel).all(), k
