"""The host-side helpers the batch engines share (engine.py, problems.py, RIPTRM.py): no GPU, no library."""
import types

import numpy as np
import pytest
import torch

import engine
import problems
from RIPTRM import RIPTRM

SIZES = [1, 255, 256, 257, 4096]


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("nbytes", SIZES)
def test_aligned_buffer_on_cpu(nbytes, zero):
    buf, addr, usable = engine.aligned_buffer(nbytes, torch.device("cpu"), zero=zero)
    assert buf.dtype == torch.uint8 and buf.device.type == "cpu"
    base, end = buf.data_ptr(), buf.data_ptr() + buf.numel()
    assert addr % 256 == 0
    assert base <= addr < end
    assert usable >= nbytes
    assert addr + usable <= end
    if zero:
        assert not buf.any()
    # the arithmetic on an existing tensor gives the same answer
    assert engine.align256(buf) == (addr, usable)


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("shift", [0, 1, 100, 255])
def test_align256_at_every_misalignment(nbytes, shift):
    """A view that starts `shift` bytes into an allocation: whatever the base address, the aligned address is
    the first multiple of 256 inside it and the usable bytes end with the view."""
    whole = torch.empty(nbytes + 256 + shift, dtype=torch.uint8)
    view = whole[shift:]
    addr, usable = engine.align256(view)
    base, end = view.data_ptr(), view.data_ptr() + view.numel()
    assert addr % 256 == 0 and base <= addr < base + 256
    assert usable >= nbytes and addr + usable == end


def test_ptr():
    assert engine.ptr(None) is None
    t = torch.arange(4, dtype=torch.float64)
    assert engine.ptr(t).value == t.data_ptr()


@pytest.mark.parametrize("make", [dict, lambda **kw: types.SimpleNamespace(**kw)], ids=["dict", "namespace"])
def test_cfg_access(make):
    cfg = make(h=0.02, name=None)
    assert problems.cfg_has(cfg, "h") and problems.cfg_has(cfg, "name") and not problems.cfg_has(cfg, "Xset")
    assert problems.cfg_get(cfg, "h") == 0.02
    assert problems.cfg_get(cfg, "h", 1.0) == 0.02
    assert problems.cfg_get(cfg, "name", "x") is None          # present: the default does not replace a None
    assert problems.cfg_get(cfg, "Xset", [1, 2]) == [1, 2]
    assert problems.cfg_get(cfg, "Xset", None) is None
    with pytest.raises(KeyError if isinstance(cfg, dict) else AttributeError):
        problems.cfg_get(cfg, "Xset")


@pytest.mark.parametrize("make", [dict, lambda **kw: types.SimpleNamespace(**kw)], ids=["dict", "namespace"])
def test_nonnegpca_coordinator_needs_its_keys(make, tmp_path):
    full = dict(problem_name="NonnegPCA", problem_instance=1, problem_initialpoint="a")
    for key in full:
        with pytest.raises(AssertionError, match=key):
            problems.Coordinator(make(**{k: v for k, v in full.items() if k != key}))
    # run() reads problem_initialpoint without a default: a cfg that lost it raises, it is not read as None
    d = tmp_path / "dataset" / "NonnegPCA" / "1"
    d.mkdir(parents=True)
    np.savetxt(d / "dim.csv", [2])
    np.savetxt(d / "Z.csv", np.eye(2))
    cfg = make(**full)
    co = problems.Coordinator(cfg, root=str(tmp_path))
    if isinstance(cfg, dict):
        del cfg["problem_initialpoint"]
    else:
        del cfg.problem_initialpoint
    with pytest.raises(KeyError if isinstance(cfg, dict) else AttributeError):
        co.run()


def test_host_array_reshapes_on_equal_count():
    batch, d = 3, 4
    flat = np.arange(batch * 3 * d * d, dtype=np.float32)
    out = engine.host_array(flat, (batch, 3, d, d))
    assert out.shape == (batch, 3, d, d) and out.dtype == np.float64
    assert np.array_equal(out.ravel(), flat)
    assert np.array_equal(engine.host_array(flat.reshape(batch, 3 * d, d).tolist(), (batch, 3, d, d)), out)
    # already of the shape: values kept, but a copy
    same = engine.host_array(out, out.shape)
    assert np.array_equal(same, out) and not np.shares_memory(same, out)


def test_host_array_broadcasts_otherwise():
    batch, m = 3, 5
    assert np.array_equal(engine.host_array(0.25, (batch,)), np.full(batch, 0.25))
    row = np.arange(m, dtype=np.float64)
    out = engine.host_array(row, (batch, m))
    assert out.shape == (batch, m) and all(np.array_equal(out[b], row) for b in range(batch))
    one = engine.host_array(7.0, (1,))                      # batch 1: count 1 either way
    assert one.shape == (1,) and one[0] == 7.0


@pytest.mark.parametrize("a, shape", [(0.5, (3,)), (np.arange(5.0), (3, 5)), (np.arange(24.0), (2, 3, 4)),
                                      (np.arange(12.0).reshape(3, 4).T, (4, 3))])
def test_host_array_is_writable_and_owns_its_data(a, shape):
    src = np.asarray(a, dtype=np.float64)
    src.setflags(write=False)
    out = engine.host_array(src, shape)
    assert out.flags.writeable and out.flags.owndata and out.flags.c_contiguous
    assert not np.shares_memory(out, src)
    out[...] = -1.0                                          # does not reach the input
    assert (np.asarray(a) != -1.0).all()
    torch.as_tensor(out)                                     # what _dev does next: no read-only warning


@pytest.mark.parametrize("a, shape", [(np.arange(4.0), (3, 5)), (np.arange(6.0), (3, 4)), (np.zeros((2, 3)), (3,))])
def test_host_array_rejects_other_shapes(a, shape):
    with pytest.raises(ValueError):
        engine.host_array(a, shape)


def test_one_launch_log_capacity():
    cap = RIPTRM.one_launch_log_capacity
    assert cap(1) == 65536 and cap(8) == 65536               # the default
    assert cap(4, 1000) == 1000 and cap(4, 100000) == 100000  # the request, while the batch's log fits
    for B in (1000, 4096, 100000):
        limit = int(RIPTRM.SI_LOG_BYTES // (256 * B))
        assert 16 <= limit < 65536
        assert cap(B) == limit and cap(B, 10 ** 9) == limit and cap(B, limit - 1) == limit - 1
    assert cap(10 ** 7) == 16 and cap(4, 3) == 16 and cap(4, 0) == 16   # the floor
    # rows that also keep a trail of 2 n k doubles (Rosenbrock with a callback) are capped tighter
    n, k, B = 30, 3, 4096
    assert cap(B, None, 256 + 16 * n * k) == int(RIPTRM.SI_LOG_BYTES // ((256 + 16 * n * k) * B)) < cap(B)
