"""The super-tile S-pass's static unit order (riptrm_device.h sup_deal_item / sup_item_unit) and the
profiling event pools across lock-step chunks.

Every unit writes its own fixed slots of the partial grid, so the order the units are dealt in can
change when a unit runs and never what it computes: the size-balanced order (RIPTRM_SUP_BALANCED=1,
read at bind) and the index order (default) must agree bit for bit.  The host mirror of the deal
(riptrm_sup_deal, the same inline functions the kernel calls) is checked on the CPU for coverage
and balance."""
import ctypes

import numpy as np
import pytest

G_CU = 256   # workgroups of a full launch: one per compute unit of the MI355X


def _engine(monkeypatch, balanced, n, B, groups=0):
    """The tests' "sym2" layout (symmetric tiles, super-tile S-pass forced), bound with the given
    unit order; the instances and the starting points are the same for every engine of one shape."""
    import engine
    monkeypatch.setenv("RIPTRM_SUP_BALANCED", "1" if balanced else "0")
    eng = engine.NonnegPCABatch(n, B, log_capacity=256, layout="sym", stream_groups=groups, spass_kind=2,
                                drain_logs=False)
    x0, y0 = eng.generate_synthetic(seed0=4100 + n)   # binds: the knob is read here
    return eng, x0, y0


@pytest.mark.gpu
@pytest.mark.parametrize("n,B", [(300, 100), (1000, 60), (129, 4), (300, 1), (2, 3)])
def test_hvp_is_bitwise_the_same_in_both_orders(monkeypatch, n, B):
    """(300, 100): 300 units, a partial second round dealt backwards; (1000, 60): 600 units, three
    rounds; (129, 4) and (300, 1): fewer units than CUs; (2, 3): one unit per instance."""
    torch = pytest.importorskip("torch")
    v = torch.from_numpy(np.random.RandomState(7 + n).randn(B, n))
    outs = []
    for balanced in (True, False):
        eng, x0, y0 = _engine(monkeypatch, balanced, n, B)
        y = y0 + 0.25 * x0
        outs.append(eng.hvp(x0, y, 0.0123, v).cpu().numpy())
        del eng
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    np.testing.assert_array_equal(outs[0], outs[1])


def _opt():
    from problems import manviofun
    return {"maxiter": 3, "tolresid": 0.0, "maxtime": 1e9, "TRS_solver": "tCG", "second_order_stationarity": False,
            "manviofun": manviofun}


@pytest.mark.gpu
def test_short_solve_is_bitwise_the_same_in_both_orders(monkeypatch):
    """n = 300, B = 100, two stream groups, 3 outer iterations: trial passes with two right-hand
    sides, lists that shrink as instances finish, both groups.  x, y and every stats field agree
    byte for byte, except RIPTRM_STAT_STOP_RUNTIME, a wall-clock reading that differs between any
    two runs."""
    pytest.importorskip("torch")
    import engine
    res = []
    for balanced in (True, False):
        eng, x0, y0 = _engine(monkeypatch, balanced, 300, 100, groups=2)
        r = eng.solve(x0, y0, _opt())
        res.append((r.x.cpu().numpy(), r.y.cpu().numpy(), np.array(r.stats, dtype=np.float64)))
        del eng
    (xa, ya, sa), (xb, yb, sb) = res
    C = engine.C
    assert (sa[:, C["RIPTRM_STAT_OUTER_ITERS"]] == 3).all() and not sa[:, C["RIPTRM_STAT_ERROR"]].any()
    assert (sa[:, C["RIPTRM_STAT_RHS"]] > sa[:, C["RIPTRM_STAT_PASSES"]]).all()   # two-right-hand-side passes ran
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(ya, yb)
    keep = [f for f in range(sa.shape[1]) if f != C["RIPTRM_STAT_STOP_RUNTIME"]]
    assert sa[:, keep].tobytes() == sb[:, keep].tobytes()


@pytest.mark.gpu
def test_profile_counts_do_not_depend_on_the_chunking(monkeypatch):
    """The timing events of a chunk are folded into the totals while the next chunk runs (two
    pools).  The same 32 lock-step iterations of the same solve, queued as 8 chunks of 4 and as one
    chunk of 32, must report the same launch counts: one S-pass and one state launch per step and
    group (no group runs empty that early, which is asserted), and positive times for both."""
    pytest.importorskip("torch")
    import engine
    STEPS = 32
    reads = []
    for chunk in (4, STEPS):
        eng, x0, y0 = _engine(monkeypatch, True, 300, 100, groups=2)
        eng.begin(x0, y0, _opt())
        engine.profile_enable(eng, True)
        for _ in range(STEPS // chunk):
            act = eng.advance(chunk)
        assert act == 100, act   # every instance of both groups still runs
        reads.append(engine.profile_read(eng))
        engine.profile_enable(eng, False)
        again = engine.profile_read(eng)
        assert again["gemv_launches"] == 0 and again["state_launches"] == 0
        del eng
    a, b = reads
    print(a, b)
    assert a["gemv_launches"] == b["gemv_launches"] == 2 * STEPS
    assert a["state_launches"] == b["state_launches"] == 2 * STEPS
    for r in reads:
        assert r["gemv_ms"] > 0 and r["state_ms"] > 0


# ---- CPU: the host side of the mapping function ------------------------------------------------

def _nsup(n):
    nst = (-(-n // 128) + 1) // 2
    return nst * (nst + 1) // 2


def _deal(lib, n, balanced, nact, grid=G_CU):
    total = nact * _nsup(n)
    wg, slot, unit = (np.full(total + 1, -1, dtype=np.int32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    cnt = lib.riptrm_sup_deal(n, 1 if balanced else 0, nact, grid, p(wg), p(slot), p(unit), total + 1)
    assert cnt == total, (n, balanced, nact, cnt, total)
    return wg[:total], slot[:total], unit[:total]


@pytest.mark.parametrize("n", [129, 300, 1000, 4000])
def test_deal_covers_every_slot_and_unit_once(built_lib, n):
    nsup = _nsup(n)
    for balanced in (True, False):
        for nact in range(1, 65):
            wg, slot, unit = _deal(built_lib, n, balanced, nact)
            assert wg.min() >= 0 and wg.max() < G_CU
            assert slot.min() >= 0 and slot.max() < nact and unit.min() >= 0 and unit.max() < nsup
            seen = np.bincount(slot.astype(np.int64) * nsup + unit, minlength=nact * nsup)
            assert (seen == 1).all(), (n, balanced, nact)


def test_deal_is_balanced_at_n4000(built_lib):
    """Heaviest workgroup's bytes over the ideal share (all bytes / 256) at n = 4000, with the
    layout's own unit sizes: never above the index order's, and <= 1.032 for 32..64 active
    instances (the bound the size-sorted back-and-forth deal was simulated to meet)."""
    n = 4000
    nsup = _nsup(n)
    size = np.array([built_lib.riptrm_sup_unit_bytes(n, u) for u in range(nsup)], dtype=np.int64)
    assert size.sum() == 8 * built_lib.riptrm_nonnegpca_s_elems(n, 1)   # the units tile the stored triangle
    assert built_lib.riptrm_sup_unit_bytes(n, nsup) == -1 and size.max() == 4 * 128 * 128 * 8
    worst = 0.0
    for nact in range(1, 65):
        ratio = {}
        for balanced in (True, False):
            wg, _, unit = _deal(built_lib, n, balanced, nact)
            load = np.bincount(wg, weights=size[unit].astype(np.float64), minlength=G_CU)
            ratio[balanced] = load.max() / (nact * size.sum() / G_CU)
        assert ratio[True] <= ratio[False] * (1 + 1e-12), (nact, ratio)
        if nact >= 32:
            worst = max(worst, ratio[True])
            assert ratio[True] <= 1.032, (nact, ratio)
    print("worst balanced ratio over 32..64 active:", worst)
