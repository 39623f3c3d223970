"""Gait-complete assembly of the controller's QP (qpb_assemble_gait), the parts that
need no GPU: the numpy restatement workloads.controller_gait_qp_from_terms of
main.cpp:1730-2005 / :2486-2695 (trot 30/70/12) and :2915-3232 (crawl 30/69/15), the
feasible synthetic terms workloads.controller_gait_terms -- every QP of every stance
mask is QP_OPTIMAL in the oracle, the condition tests/test_gpu_gait_assemble.py
relies on -- and the argument checks of the C entry point, which run before any HIP
call."""
import ctypes as C

import numpy as np
import pytest

from apf_quadruped_amd import workloads as W

SEED = 0xD06B07 + 60
TROT, CRAWL = (0xA, 0x5), (0xE, 0xB, 0xD, 0x7)
# (mask, trot_b_dynamics): the flag has no effect outside trot, so one mode there
CASES = [(0xF, False)] + [(s, f) for s in TROT for f in (False, True)] + [(s, False) for s in CRAWL]
QPB_OK, QPB_EINVAL, QPB_ESHAPE = 0, -1, -5


def test_stance_mask_is_the_stance_restatement():
    t = W.controller_gait_terms(SEED, np.arange(5), 0xF)
    d, ref = W.controller_gait_qp_from_terms(t, 0xF), W.controller_qp_from_terms(t)
    assert (d["n"], d["m"], d["p"]) == (30, 68, 18)
    for k in ("P", "A", "G", "c", "h", "b"):
        assert np.array_equal(d[k], ref[k]), k
    d = W.controller_gait_qp_from_terms(t, 0xF, mu=0.7, trot_b_dynamics=True)
    ref = W.controller_qp_from_terms(t, 0.7)
    for k in ("P", "A", "G", "c", "h", "b"):
        assert np.array_equal(d[k], ref[k]), k


@pytest.mark.parametrize("stance", TROT + CRAWL)
def test_shapes_slack_weights_and_layout(stance):
    B = 4
    t = W.controller_gait_terms(SEED + 1, np.arange(B), stance)
    d = W.controller_gait_qp_from_terms(t, stance)
    trot = stance in TROT
    assert (d["n"], d["m"], d["p"]) == ((30, 70, 12) if trot else (30, 69, 15))
    assert d["P"].shape == (B, 30, 30) and d["A"].shape == (B, d["p"], 30) and d["G"].shape == (B, d["m"], 30)
    k = 2 if trot else 3
    o_s, nw, r0 = 18 + 3 * k, 12 - 3 * k, 5 * k
    diag = np.diagonal(d["P"], axis1=1, axis2=2)
    assert np.array_equal(diag[:, o_s:], np.full((B, nw), 1e8 if trot else 1e4))
    assert np.array_equal(diag[:, :18], np.ones((B, 18)))
    st = [i for i in range(4) if (stance >> i) & 1]
    sw = [i for i in range(4) if i not in st]
    rs = np.array([3 * i + a for i in st for a in range(3)])
    rw = np.array([3 * i + a for i in sw for a in range(3)])
    # stance / swing rows of Jst in ascending foot order, signs and slack columns
    assert np.array_equal(d["A"][:, 6:, 0:18], t["Jst"][:, rs, :])
    assert np.array_equal(d["A"][:, 0:6, 18:o_s], -np.transpose(t["Jst"][:, rs, 0:6], (0, 2, 1)))
    r1 = r0 + 24
    assert np.array_equal(d["G"][:, r1:r1 + nw, 0:18], t["Jst"][:, rw, :])
    assert np.array_equal(d["G"][:, r1 + nw:r1 + 2 * nw, 0:18], -t["Jst"][:, rw, :])
    for half in (0, 1):
        assert np.array_equal(d["G"][:, r1 + half * nw:r1 + (half + 1) * nw, o_s:],
                              np.broadcast_to(-np.eye(nw), (B, nw, nw)))
    v = (t["sw_acc"][:, rw] + 20.0 * t["sw_vel"][:, rw]) + 300.0 * t["sw_pos"][:, rw]
    assert np.array_equal(d["h"][:, r1:r1 + nw], v - t["jdqd"][:, rw])
    assert np.array_equal(d["h"][:, r1 + nw:r1 + 2 * nw], -d["h"][:, r1:r1 + nw])
    assert np.array_equal(d["h"][:, :r0], np.zeros((B, r0)))
    assert W.pack_swing(t).shape == (B, W.SWING_NV) and W.SWING_NV == 36
    assert np.array_equal(W.pack_swing(t)[:, 12:24], t["sw_pos"])


@pytest.mark.parametrize("stance", TROT + CRAWL)
def test_equality_right_hand_side(stance):
    B = 4
    t = W.controller_gait_terms(SEED + 2, np.arange(B), stance)
    st = [i for i in range(4) if (stance >> i) & 1]
    rs = np.array([3 * i + a for i in st for a in range(3)])
    dyn = np.concatenate([-t["bias"][:, 0:6], -t["jdqd"][:, rs]], 1)
    b0 = W.controller_gait_qp_from_terms(t, stance)["b"]
    b1 = W.controller_gait_qp_from_terms(t, stance, trot_b_dynamics=True)["b"]
    assert np.array_equal(b1, dyn)
    if stance in TROT:
        assert np.array_equal(b0, np.zeros((B, 12))) and np.abs(dyn).min() > 0.0
    else:
        assert np.array_equal(b0, dyn)


def test_bad_masks_are_refused_by_the_restatement():
    t = W.controller_gait_terms(SEED, np.arange(1), 0xF)
    for bad in (0x0, 0x1, 0x2, 0x4, 0x8, 0x3, 0x6, 0x9, 0xC, 0x10, -1):
        with pytest.raises(ValueError):
            W.controller_gait_qp_from_terms(t, bad)


@pytest.mark.parametrize("stance,dyn", CASES)
def test_gait_terms_are_optimal_in_the_oracle(stance, dyn, oracle):
    """96 QPs per mask and trot b mode, the reference's AMD order (perm = NULL):
    QP_OPTIMAL at the controller's tolerance and at 1e-6."""
    B = 96
    t = W.controller_gait_terms(SEED + 3, np.arange(B), stance)
    d = W.controller_gait_qp_from_terms(t, stance, trot_b_dynamics=dyn)
    Pc, Ac, Gc = W.to_colmajor(d["P"]), W.to_colmajor(d["A"]), W.to_colmajor(d["G"])
    for tol in (1e-2, 1e-6):
        _, flags, iters = oracle.solve_dense_batch(30, d["m"], d["p"], Pc, Ac, Gc, d["c"], d["h"], d["b"],
                                                   reltol=tol, abstol=tol)
        assert (flags == 0).all(), (hex(stance), dyn, tol, np.flatnonzero(flags))
        assert iters.max() < 50
    # one sparsity pattern per mask
    for k in ("P", "A", "G"):
        assert ((d[k] != 0.0) == (d[k][0] != 0.0)[None]).all(), k


def _plan(stance):
    from apf_quadruped_amd.batch import Plan
    d = W.controller_gait_qp_from_terms(W.controller_gait_terms(SEED + 4, np.arange(1), stance), stance)
    return Plan.from_dense(30, d["m"], d["p"], d["P"][0], d["A"][0], d["G"][0])


def _call(plan, B, stance, flags=0, data=None, swing=None):
    """qpb_assemble_gait with `data` for every required pointer (NULL by default)."""
    from apf_quadruped_amd import _lib
    h = plan._h if plan is not None else None
    return _lib.lib().qpb_assemble_gait(h, B, stance, data, 0, None, swing, 0, 0.5, flags, data, data, data, data, data,
                                        data, None, None)


def test_argument_checks_need_no_gpu():
    """Checked before any HIP call, in the documented order: NULL plan, mask and flags
    (QPB_EINVAL), shape (QPB_ESHAPE), B = 0 (QPB_OK), NULL data (QPB_EINVAL)."""
    plans = {s: _plan(s) for s in (0xF, 0xA, 0xE)}
    assert _call(None, 0, 0xF) == QPB_EINVAL
    for bad in (0x0, 0x1, 0x2, 0x4, 0x8, 0x3, 0x6, 0x9, 0xC, 0x10, 0x1F, -1):
        for plan in plans.values():
            assert _call(plan, 0, bad) == QPB_EINVAL, hex(bad)
    for flags in (0x2, 0x3, 0x100, -1):
        assert _call(plans[0xA], 0, 0xA, flags=flags) == QPB_EINVAL
    # a bad mask is reported before the shape it could not have matched
    assert _call(plans[0xA], 0, 0x3) == QPB_EINVAL
    good = {0xF: (0xF,), 0xA: TROT, 0xE: CRAWL}
    for key, plan in plans.items():
        for stance in (0xF,) + TROT + CRAWL:
            want = QPB_OK if stance in good[key] else QPB_ESHAPE
            assert _call(plan, 0, stance) == want, (hex(key), hex(stance))
            assert _call(plan, 0, stance, flags=0x1) == want            # the flag is accepted in every phase
    # the shape is checked before B = 0 and before the data pointers
    assert _call(plans[0xA], 7, 0xE) == QPB_ESHAPE
    assert _call(plans[0xA], -1, 0xA) == QPB_EINVAL
    # NULL data with B > 0: refused without touching the GPU
    buf = (C.c_double * 8)()
    ptr = C.cast(buf, C.c_void_p)
    assert _call(plans[0xA], 3, 0xA) == QPB_EINVAL
    assert _call(plans[0xE], 3, 0xE, data=ptr, swing=None) == QPB_EINVAL     # swing required off 0xF
    assert _call(plans[0xF], 3, 0xF) == QPB_EINVAL
    from apf_quadruped_amd import _lib
    assert b"NULL data pointer" in _lib.lib().qpb_last_error()
