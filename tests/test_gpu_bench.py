"""bench.py's plain run end to end, at a tiny size: it times --steps steps,
prints one result line with ms_per_step, leaves what takes runs of its own
(serialised rooflines, exact-fp32 leg, CPU baselines) to --full, and
--dump-outputs writes the last timed step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, I = 256, 64, 128


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--batch", str(B), "--img", "32", "--poses", "2",
                        "--dump-outputs", str(out)],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["full"] is False
    assert j["unit"] == "rays/s" and j["higher_is_better"] is True and j["dtype"] == "f16x3"
    assert j["ms_per_step"] > 0
    # value and ms_per_step state the same timed region (both rounded in the line)
    assert j["value"] == pytest.approx(B / (j["ms_per_step"] * 1e-3), rel=2e-3)
    # the kernels of exactly the 3 timed steps: one coarse and one fine forward each
    assert j["kernels"]["mlp_fwd"]["launches"] == 2 * 3
    for k in ("fp32_leg", "cpu_baseline", "cpu_baseline_1thread", "rooflines_concurrent"):
        assert j[k] is None, k
    assert j["rooflines_basis"] == "the timed region"
    want = {"rgb_coarse": (B, 3), "depth_coarse": (B,), "opacity_coarse": (B,), "rgb_fine": (B, 3),
            "depth_fine": (B,), "opacity_fine": (B,), "loss": (1,), "params_coarse": (595844,),
            "params_fine": (595844,)}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    for k, shape in want.items():
        v = np.load(out / (k + ".npy"), allow_pickle=False)
        assert v.dtype == np.float32 and v.shape == shape and np.isfinite(v).all(), k
    assert float(np.load(out / "loss.npy")[0]) == pytest.approx(j["final_loss"], abs=1e-5)
