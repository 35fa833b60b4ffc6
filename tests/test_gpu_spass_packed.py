"""The super-tile S-pass streaming S from its exact 58-bit packed copy (csrc/riptrm_spack.h) against
the same kernel on plain S.  The decode gives every double back bit for bit and every FMA, reduction
and store keeps its place, so results must be equal byte for byte: assert_array_equal, no tolerance.

RIPTRM_SPASS_PACKED is read at bind (1: every symmetric-tile bind, 0: never, unset: from n = 2561
on, where the automatic rule streams with k_spass_sup); RIPTRM_SPACK_VERIFY=1 makes bind decode
every packed tile on the device and count the elements that differ from plain S."""
import numpy as np
import pytest

from oracle.nonnegpca_gen import SEED0, generate_instance

TS = 128


def _tiles(n):
    """(stored tiles, full tiles) of one symmetric-tile instance."""
    nt = -(-n // TS)
    wl = -(-(n - (nt - 1) * TS) // 32) * 32
    ntf = nt if wl == TS else nt - 1
    return nt * (nt + 1) // 2, ntf * (ntf + 1) // 2


def _env(monkeypatch, packed):
    monkeypatch.setenv("RIPTRM_SPACK_VERIFY", "1")
    if packed is None:
        monkeypatch.delenv("RIPTRM_SPASS_PACKED", raising=False)
    else:
        monkeypatch.setenv("RIPTRM_SPASS_PACKED", "1" if packed else "0")


def _engine(monkeypatch, packed, n, B, groups=0, kind=2):
    import engine
    _env(monkeypatch, packed)
    eng = engine.NonnegPCABatch(n, B, log_capacity=256, layout="sym", stream_groups=groups, spass_kind=kind,
                                drain_logs=False)
    x0, y0 = eng.generate_synthetic(seed0=4100 + n)   # binds: the knobs are read here
    return eng, x0, y0


def _hvp(eng, x0, y0, v):
    out = eng.hvp(x0, y0 + 0.25 * x0, 0.0123, v).cpu().numpy()
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n,B", [(129, 4), (300, 100), (1000, 60), (2, 3)])
def test_hvp_is_bitwise_the_same_packed_and_plain(monkeypatch, n, B):
    """(129, 4): one full tile plus 32-wide edge tiles; (300, 100): partial last super-block, more
    units than CUs; (1000, 60): every tile full, the last ones zero-padded (zeros are code 0);
    (2, 3): no full tile, so no packed copy at all."""
    torch = pytest.importorskip("torch")
    v = torch.from_numpy(np.random.RandomState(7 + n).randn(B, n))
    stored, full = _tiles(n)
    outs = []
    for packed in (True, False):
        eng, x0, y0 = _engine(monkeypatch, packed, n, B)
        info = eng.spass_packed_info()
        print(n, B, packed, info)
        if packed and full:
            assert info["in_use"] and info["verify_mismatches"] == 0
            assert info["tiles_packed"] == B * full and info["tiles_plain"] == B * (stored - full)
            assert info["bytes"] >= B * full * 118784
        else:
            assert info == {"in_use": False, "tiles_packed": 0, "tiles_plain": B * stored, "bytes": 0,
                            "verify_mismatches": -1}
        outs.append(_hvp(eng, x0, y0, v))
        del eng
    np.testing.assert_array_equal(outs[0], outs[1])


def _opt():
    from problems import manviofun
    return {"maxiter": 3, "tolresid": 0.0, "maxtime": 1e9, "TRS_solver": "tCG", "second_order_stationarity": False,
            "manviofun": manviofun}


@pytest.mark.gpu
def test_short_solve_is_bitwise_the_same_packed_and_plain(monkeypatch):
    """n = 300, B = 100, two stream groups, 3 outer iterations: trial passes with two right-hand sides
    (decoded once, used twice), lists that shrink as instances finish, both groups.  x, y and every
    stats field but the wall-clock RIPTRM_STAT_STOP_RUNTIME agree byte for byte."""
    pytest.importorskip("torch")
    import engine
    res = []
    for packed in (True, False):
        eng, x0, y0 = _engine(monkeypatch, packed, 300, 100, groups=2)
        assert eng.spass_packed_info()["in_use"] == packed
        r = eng.solve(x0, y0, _opt())
        res.append((r.x.cpu().numpy(), r.y.cpu().numpy(), np.array(r.stats, dtype=np.float64)))
        if packed:
            assert eng.spass_packed_info()["verify_mismatches"] == 0
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
def test_escapes_zeros_denormals_and_a_far_base(monkeypatch):
    """Instance 0: the recipe.  Instance 1: S is exactly 2^-60 at one off-diagonal pair inside tile
    (0, 0), far below what a 5-bit code reaches, so that tile stays plain; tile (0, 1) holds a handful
    of exact zeros and one denormal, which are code 0, so it packs.  Instance 2: the recipe times
    2^40, packed through its tiles' own bases.  One more plain tile than the edges, and hvp equal to
    the plain engine bit for bit."""
    torch = pytest.importorskip("torch")
    import engine
    n, B = 300, 3
    Z = np.stack([generate_instance(n, SEED0 + b)[0] for b in range(B)])
    Z[1, 3, 10] = Z[1, 10, 3] = 2.0 ** -61
    for i, j in [(0, 128), (5, 130), (77, 255), (127, 201), (64, 192)]:
        Z[1, i, j] = Z[1, j, i] = 0.0
    Z[1, 9, 140], Z[1, 140, 9] = 5e-324 * 12345, 0.0
    Z[2] *= 2.0 ** 40
    S1 = Z[1] + Z[1].T
    assert S1[3, 10] == 2.0 ** -60 and S1[9, 140] == 5e-324 * 12345 and S1[5, 130] == 0.0 and np.isfinite(Z).all()
    rs = np.random.RandomState(5)
    x = np.abs(rs.randn(B, n)) + 0.1
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = 1.0 + rs.rand(B, n)
    v = rs.randn(B, n)
    stored, full = _tiles(n)
    outs = []
    for packed in (True, False):
        _env(monkeypatch, packed)
        eng = engine.NonnegPCABatch(n, B, log_capacity=16, layout="sym", spass_kind=2, drain_logs=False)
        eng.load_Z(Z)
        info = eng.spass_packed_info()
        print(packed, info)
        if packed:
            assert info["in_use"] and info["verify_mismatches"] == 0
            assert info["tiles_plain"] == B * (stored - full) + 1 and info["tiles_packed"] == B * full - 1
        out = eng.hvp(x, y, 0.0123, v).cpu().numpy()
        assert np.isfinite(out).all()
        outs.append(out)
        del eng
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.gpu
def test_packing_into_a_bound_S_refreshes_the_copy(monkeypatch):
    """riptrm_nonnegpca_pack into the bound S (no new bind) repacks the instance it wrote: the packed
    copy is never stale."""
    torch = pytest.importorskip("torch")
    n, B = 300, 2
    v = torch.from_numpy(np.random.RandomState(3).randn(B, n))
    Znew = torch.from_numpy(generate_instance(n, SEED0 + 40)[0])
    outs = []
    for packed in (True, False):
        eng, x0, y0 = _engine(monkeypatch, packed, n, B)
        before = _hvp(eng, x0, y0, v)
        eng.pack_one(Znew.to(eng.device).contiguous(), 1)
        after = _hvp(eng, x0, y0, v)
        assert (before[0] == after[0]).all() and (before[1] != after[1]).any()
        if packed:
            assert eng.spass_packed_info()["verify_mismatches"] == 0
        outs.append(after)
        del eng
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.gpu
def test_default_rule(monkeypatch):
    """Knob unset: a packed copy exactly where the automatic rule streams with k_spass_sup (n >= 2561)."""
    torch = pytest.importorskip("torch")
    eng, _, _ = _engine(monkeypatch, None, 300, 4, kind=1)
    assert not eng.spass_packed_info()["in_use"]
    del eng
    n, B = 2600, 2
    stored, full = _tiles(n)
    v = torch.from_numpy(np.random.RandomState(9).randn(B, n))
    outs = []
    for packed in (None, False):
        eng, x0, y0 = _engine(monkeypatch, packed, n, B, kind=1)
        info = eng.spass_packed_info()
        assert eng.spass_calibration()["kernel"] == "k_spass_sup"
        assert info["in_use"] == (packed is None)
        if packed is None:
            assert info["verify_mismatches"] == 0 and info["tiles_packed"] == B * full
        outs.append(_hvp(eng, x0, y0, v))
        del eng
    np.testing.assert_array_equal(outs[0], outs[1])
