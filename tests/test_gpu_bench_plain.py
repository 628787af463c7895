"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run times its K steps and nothing else, and
`--dump-outputs DIR` writes the P of the last timed step (DIR/P.npy, float32, CSR order), equal
by the checkData rule to the oracle's host SDDMM on the same operands. With `--full` the line
carries the legs that moved out of the plain run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from bsmr import make_data, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra, **env_extra):
    env = dict(os.environ, **env_extra)
    for k in ("BSMR_DIST_BACKEND", "WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7",
           "--warmup", "2"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0])


def test_full_run_carries_the_moved_legs():
    """`--full` on one GPU (C2; the PMC child processes left out): the legs a plain run no longer
    has are in the line, and the baselines agree with the engine's P."""
    out = _bench("--full", "--pmc", "off", OMP_NUM_THREADS="4")
    assert out["full"] is True and out["steps"] == 7 and out["ms_per_step"] > 0
    assert out["cold"]["ms_per_step"] > 0 and out["cold"]["clean"]["ms_per_step"] > 0
    assert out["kernels_ms"]["total_ms"] > 0 and out["kernels_ms"]["residual_ms"] > 0
    assert out["mfma"]["forced_tiles_split"]["checkData_errors_vs_line"] == 0
    assert out["vendor_baseline"]["value"] > 0
    assert out["vendor_baseline"]["default"]["checkData_errors_vs_engine"] == 0
    assert out["cpu_baseline"]["value"] > 0
    assert out["cpu_baseline"]["checkData_errors_vs_gpu"] == 0


def test_plain_run_is_lean_and_dumps_the_timed_P(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    assert out["steps"] == 7 and out["warmup"] == 2 and out["full"] is False
    assert out["unit"] == "GFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    nnz, K = out["config"]["nnz"], out["config"]["K"]
    assert out["value"] == pytest.approx(2.0 * nnz * K / (out["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    # the graph of the 7 launches, when it was the timed form, wrote the stream-launched P
    if out["timing"]["method"] == "hip_graph":
        assert out["timing"]["graph_P_mismatches_vs_stream"] == 0
    else:
        assert out["timing"]["method"] == "stream_launches" and out["timing"]["graph_error"]
    # none of the --full legs ran
    for leg in ("cpu_baseline", "vendor_baseline", "cold"):
        assert leg not in out, leg
    assert out["kernels_ms"] == {} and out["roofline"]["traffic"] is None
    assert sorted(os.listdir(tmp_path)) == ["P.npy"]
    P = np.load(tmp_path / "P.npy")
    M, N, rp, ci = synth.nips_like()
    assert P.dtype == np.float32 and P.shape == (nnz,) and nnz == len(ci)
    ref = O.sddmm_cpu(O.CSR.from_arrays(M, N, rp, ci), K, make_data(M * K), make_data(N * K))
    assert O.check_data(ref, P) == 0
