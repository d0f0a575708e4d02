"""GPU (-m gpu): a plain bench.py run on a small table -- the headline line alone, and --dump-outputs writing what the timed steps left in the table."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rustsolver_amd as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need a real MI355X (there is no CPU fallback)")


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_dumps_the_table_the_timed_steps_left(tmp_path):
    """`bench.py --boards 64 --steps 3 --warmup 2 --dump-outputs DIR`: one JSON line with the contract keys and no --full leg; the dumped sample equals
    the same trainer's table after warmup + steps iterations, built and swept in this process"""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--boards", "64", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(dump), "--detail", str(tmp_path / "detail.json")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == "cfr_iterations_per_sec" and out["unit"] == "board-iterations/s" and out["higher_is_better"] is True and out["dtype"] == "i32"
    assert out["steps"] == 3 and out["warmup"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 64 * 3 / (out["ms_per_step"] * 3e-3)) <= 1e-3 * out["value"]
    assert not any(k in out for k in ("roofline", "cpu_baseline", "config3", "deal_batch", "solve_s"))

    b = load_bench()
    trainer = b.make_trainer(rs, 64, 1000, "clamp", 0, 0, 1234 + 1, -1, "river", "i32", "full", None, saturating=100)
    try:
        b.run_steps(trainer, 2 + 3)
        b.dump_outputs(trainer.infosets, str(tmp_path / "here"))
    finally:
        trainer.destroy()
        trainer.infosets.destroy()
    for name in ("regrets", "strategy_sum"):
        got, want = np.load(str(dump / (name + ".npy"))), np.load(str(tmp_path / "here" / (name + ".npy")))
        assert got.dtype == np.float64 and got.size > 0 and np.array_equal(got, want), name
