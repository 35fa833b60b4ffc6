"""bench.py on the GPU at a small size (a graph-replayed batch): the plain run times `--steps` steps
and reports the headline fields with nothing of `--full` (no CPU baseline, no second profiled
window); `--full` adds the roofline from its second window; `--dump-outputs` writes the x / y the last
timed step left, the same from run to run, with or without `--full`, and equal to a direct engine
solve of the same instances."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B, W, K, SEED0 = 200, 4, 1, 3, 20251212


def _bench(extra, dump_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dim", str(N), "--batch", str(B),
                        "--warmup", str(W), "--steps", str(K), "--dump-outputs", str(dump_dir)] + extra,
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    assert sorted(os.listdir(dump_dir)) == ["x.npy", "y.npy"]
    return json.loads(lines[0]), {k: np.load(os.path.join(dump_dir, f"{k}.npy")) for k in ("x", "y")}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench([], tmp_path_factory.mktemp("plain"))


def _headline(out):
    assert out["steps"] == K and out["warmup"] == W
    assert out["config"]["outer_window"] == [W + 1, W + K]
    assert out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f64"
    # value = outer iterations of the whole batch over the timed seconds: B per step
    assert out["value"] == pytest.approx(B / (out["ms_per_step"] / 1e3), rel=1e-9)


def test_plain_run_headline_without_the_full_parts(plain):
    out, dump = plain
    _headline(out)
    assert out["cpu_baseline"] is None                     # --full's
    assert out["roofline"] is None                         # a small batch replays graphs: profiled by --full only
    assert out["detail"]["gemv_launches"] is None and out["detail"]["state_kernel_ms"] is None
    for k in ("x", "y"):
        assert dump[k].dtype == np.float64 and dump[k].shape == (B, N)


@pytest.mark.parametrize("extra", [[], ["--full", "--cpu-budget", "0"]], ids=["plain", "full"])
def test_dump_repeats_bit_for_bit(plain, extra, tmp_path):
    out, dump = _bench(extra, tmp_path)
    _headline(out)
    if extra:   # the second, profiled window ran (after the dump's state was taken) and priced a kernel
        assert out["roofline"] is not None and out["roofline"]["kernel"]
        assert out["detail"]["state_launches"] > 0
        assert out["cpu_baseline"] is None                 # --cpu-budget 0
    for k in ("x", "y"):
        np.testing.assert_array_equal(dump[k], plain[1][k], err_msg=k)


def test_dump_equals_engine_solve(plain):
    import engine
    from problems import manviofun
    eng = engine.NonnegPCABatch(N, B, log_capacity=64, layout="sym", drain_logs=False)
    xg, yg = eng.generate_synthetic(SEED0, ids=list(range(B)))
    opt = {"maxiter": W + 2 * K, "tolresid": 0.0, "maxtime": float("inf"), "manviofun": manviofun,
           "TRS_solver": "tCG", "second_order_stationarity": False}
    eng.begin(xg, yg, opt, restart_every=20)
    eng.run_until(W + K)
    res = eng.result()
    np.testing.assert_array_equal(plain[1]["x"], res.x.cpu().numpy()[:, :N])
    np.testing.assert_array_equal(plain[1]["y"], res.y.cpu().numpy()[:, :N])
