"""The exact 58-bit packed copy of S (csrc/riptrm_spack.h) on the CPU, through the library's host
mirrors: the same inline functions the pack kernel and the super-tile S-pass call.

An element keeps its low dword, its sign and its top 20 mantissa bits and replaces the 11-bit exponent
field by a 5-bit code against a per-tile base (code 0 = exponent field 0), so a block of 16 rows x
128 columns round-trips bit for bit or is refused.  Bit patterns are compared through uint64 views:
-0.0 == +0.0 and NaN != NaN would hide exactly the cases that matter."""
import ctypes

import numpy as np
import pytest

from oracle.nonnegpca_gen import SEED0, generate_instance

BLOCK_BYTES = 14848
ROWS, TS = 16, 128


def _bits(sign, expo, mant):
    """The double with this sign, biased exponent field and 52-bit mantissa."""
    return np.array([(sign << 63) | (expo << 52) | mant], dtype=np.uint64).view(np.float64)[0]


def _encode(lib, rows, ebase):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    assert rows.shape == (ROWS, TS)
    out = np.full(BLOCK_BYTES + 64, 0xA5, dtype=np.uint8)   # guard bytes behind the block
    rc = lib.riptrm_spack_encode_block(rows.ctypes.data_as(ctypes.c_void_p), ebase, out.ctypes.data_as(ctypes.c_void_p))
    assert (out[BLOCK_BYTES:] == 0xA5).all()
    return rc, out


def _decode(lib, blk, ebase):
    rows = np.full((ROWS, TS), np.nan)
    assert lib.riptrm_spack_decode_block(blk.ctypes.data_as(ctypes.c_void_p), ebase, rows.ctypes.data_as(ctypes.c_void_p)) == 0
    return rows


def _classify(lib, v):
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    rng = (ctypes.c_int32 * 3)()
    word = lib.riptrm_spack_classify(v.ctypes.data_as(ctypes.c_void_p), v.size, rng)
    return word, tuple(rng)


def _round_trip(lib, rows, ebase):
    rc, blk = _encode(lib, rows, ebase)
    assert rc == 0
    back = _decode(lib, blk, ebase)
    np.testing.assert_array_equal(back.view(np.uint64), np.ascontiguousarray(rows).view(np.uint64))


def test_gaussian_block_round_trips(built_lib):
    n = 4000
    rows = np.random.RandomState(3).randn(ROWS, TS) * np.sqrt(2.0 / n)
    word, (emin, emax, bad) = _classify(built_lib, rows)
    expo = (rows.view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7FF
    assert (emin, emax, bad) == (expo.min(), expo.max(), 0) and word == emax - 31
    _round_trip(built_lib, rows, word)


def test_special_values_round_trip(built_lib):
    """+-0, denormals (smallest, largest, a middle one), the smallest and the largest exponent a base
    can carry with all-zero and all-one mantissas, both signs; dealt over the block with a stride
    coprime to its shape so that every value meets many lane positions."""
    ebase = 1000
    ones = (1 << 52) - 1
    vals = []
    for sign in (0, 1):
        vals += [_bits(sign, 0, 0), _bits(sign, 0, 1), _bits(sign, 0, ones), _bits(sign, 0, 0x000F0F0F0F0F0F)]
        for expo in (ebase + 1, ebase + 31, ebase + 17):
            vals += [_bits(sign, expo, 0), _bits(sign, expo, ones), _bits(sign, expo, 0x5A5A5A5A5A5A5 & ones)]
    vals = np.array(vals)
    for shift in range(len(vals)):
        rows = vals[(np.arange(ROWS * TS) * 7 + shift) % len(vals)].reshape(ROWS, TS)
        _round_trip(built_lib, rows, ebase)


def test_every_lane_position_with_both_signs(built_lib):
    """A lane's 32 elements are 32 fields of 26 bits in a 26-dword stream, so most fields straddle a
    dword boundary.  For each of the 32 positions (row 8 rb + k, column parity c) and both signs: the
    position alone holds an all-ones field (largest code, mantissa ones) among +0.0, then the
    position alone holds zero among all-ones fields: a bit that leaks into, or is lost from, a
    neighbouring field shows either way."""
    ebase = -7   # bases may be negative: tiles whose largest exponent field is below 31
    big = {s: _bits(s, ebase + 31, (1 << 52) - 1) for s in (0, 1)}
    for e in range(32):
        r, c = 8 * (e >> 4) + ((e >> 1) & 7), e & 1
        for s in (0, 1):
            rows = np.zeros((ROWS, TS))
            rows[r, c::2] = big[s]
            _round_trip(built_lib, rows, ebase)
            rows = np.full((ROWS, TS), big[1 - s])
            rows[r, c::2] = _bits(s, 0, 0)
            _round_trip(built_lib, rows, ebase)


def test_encode_refuses_what_the_base_cannot_carry(built_lib):
    ebase = 1000
    for bad in (_bits(0, ebase, 5), _bits(1, ebase + 32, 0), _bits(0, 5, 0), np.inf, -np.inf, np.nan):
        rows = np.full((ROWS, TS), _bits(0, ebase + 3, 99))
        rows[9, 77] = bad
        assert _encode(built_lib, rows, ebase)[0] == -1


def test_classifier(built_lib):
    rs = np.random.RandomState(11)
    tile = (1.0 + rs.rand(TS, TS)) * 2.0 ** -5 * np.where(rs.rand(TS, TS) < 0.5, -1.0, 1.0)
    word, (emin, emax, bad) = _classify(built_lib, tile)
    assert word == 1023 - 5 - 31 and (emin, emax, bad) == (1018, 1018, 0)
    t = tile.copy()
    t[100, 3] = 2.0 ** -60          # 55 binades below its neighbours: no 5-bit code reaches it
    assert _classify(built_lib, t)[0] == 0
    t[100, 3] = 2.0 ** -35          # exactly 30 binades below the largest: code 1, the last that packs
    assert _classify(built_lib, t)[0] == word
    t[100, 3] = 2.0 ** -36
    assert _classify(built_lib, t)[0] == 0
    for v in (np.inf, -np.inf, np.nan):
        t = tile.copy()
        t[5, 120] = v
        w, (_, _, bad) = _classify(built_lib, t)
        assert w == 0 and bad == 1
    # zeros and denormals take code 0 whatever the base: a tile of nothing else packs, and so does a
    # tile that mixes them with normal numbers
    t = np.zeros((TS, TS))
    t[::3, ::5] = 5e-324
    t[1::3, ::7] = -2.0 ** -1060
    t[2, 2] = -0.0
    w, rng = _classify(built_lib, t)
    assert w != 0 and rng == (0x7FF, 0, 0)
    _round_trip(built_lib, t[:ROWS], w)
    t2 = tile.copy()
    t2[::3, ::5] = 0.0
    t2[7, 7] = 5e-324
    assert _classify(built_lib, t2)[0] == word
    _round_trip(built_lib, t2[:ROWS], word)


def test_reference_recipe_tiles_all_pack(built_lib):
    """A condition on the recipe, not a measurement: every full tile of S = Z + Z^T packs, for
    generate_instance(300, SEED0 .. SEED0 + 7), and its blocks round-trip."""
    n = 300
    for s in range(SEED0, SEED0 + 8):
        Z, _, _ = generate_instance(n, s)
        S = Z + Z.T
        for I in range(2):
            for J in range(I, 2):
                tile = np.ascontiguousarray(S[I * TS:(I + 1) * TS, J * TS:(J + 1) * TS])
                word, (emin, emax, bad) = _classify(built_lib, tile)
                assert word != 0 and word == emax - 31 and emin > word and bad == 0, (s, I, J, emin, emax)
                _round_trip(built_lib, tile[3 * ROWS:4 * ROWS], word)


def test_size_arithmetic(built_lib):
    lib = built_lib
    assert lib.riptrm_spack_tile_bytes() == 118784 == 8 * BLOCK_BYTES
    assert lib.riptrm_spack_pass_bytes(4000) == 59940864
    plain = 8 * lib.riptrm_nonnegpca_s_elems(4000, 1)
    assert plain == 66035712 and plain - 59940864 == 496 * (131072 - 118784)
    assert lib.riptrm_spack_pass_bytes(300) == 8 * lib.riptrm_nonnegpca_s_elems(300, 1) - 3 * 12288
    assert lib.riptrm_spack_pass_bytes(2) == 8 * lib.riptrm_nonnegpca_s_elems(2, 1)    # no full tile
    assert lib.riptrm_spack_pass_bytes(256) == 3 * 118784                               # no edge tile
