"""bench.py's command line on the GPU (needs an MI355X): a plain run does the timed steps only,
--steps sets their number even past the end of phase 1, and --dump-outputs writes the state the
last timed step left -- the same from run to run, and bit for bit the CPU oracle's.

Config 2 (generateRandomProblem(2048, 1024, 205824, 1, 100), 32-pivot batches; 2003 phase-1 pivots,
tests/golden/published_pivots.json) keeps each bench process to a few seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, SEED, K, P1 = 2048, 1024, 205824, 32, 2003


def run_bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SIMPLEX_GPUS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "config2", *args],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_oracles_state(gpu, tmp_path):
    import oracle

    steps, warmup = 3, 1
    lines, dumps = [], []
    for name in ("a", "b"):
        d = tmp_path / name
        lines.append(run_bench("--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(d)))
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    line = lines[0]
    # the plain line: the headline figures, and nothing that takes a run of its own
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["config"]["pivots_timed"] == steps * K and line["config"]["laps"] == 1
    assert line["unit"] == "pivots/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(steps * K / (line["ms_per_step"] * steps / 1e3))
    assert line["roofline"]["timed_launches"] == steps
    for moved in ("secondary", "update_bench", "full_solve"):
        assert moved not in line
    assert line["cpu_baseline"] is None and line["parity"] is None
    # the dump: float64 arrays, under 64 MB in all, identical from run to run
    assert sorted(dumps[0]) == ["basis", "objective_row", "pivots_and_status", "tableau"]
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20
    for name, a in dumps[0].items():
        assert a.dtype == np.float64
        assert np.array_equal(a.view(np.uint64), dumps[1][name].view(np.uint64)), name
    # and the oracle's state after the same (warmup + steps) * K pivots, bit for bit
    A, b, c = oracle.generate(N, M, SEED, 1, 100)
    T, d, base = oracle.build_phase1(A, b)
    oracle.update_objective(T, d, base)
    _, done = oracle.solve(T, d, base, max_pivots=(warmup + steps) * K)
    assert done == (warmup + steps) * K
    got = dumps[0]
    assert list(got["pivots_and_status"]) == [done, line["config"]["status_after"]]
    assert np.array_equal(got["tableau"].view(np.uint64), T.view(np.uint64))
    assert np.array_equal(got["objective_row"].view(np.uint64), d.view(np.uint64))
    assert np.array_equal(got["basis"], base.astype(np.float64))


def test_steps_past_the_end_of_phase_one_are_timed_in_laps(gpu):
    """70 steps after 2 untimed ones: the first lap has 2003 - 64 pivots left (61 steps, the last
    one short), the second lap times the other 9."""
    line = run_bench("--steps", "70", "--warmup", "2")
    assert line["steps"] == 70 and line["config"]["laps"] == 2
    assert line["config"]["pivots_timed"] == (P1 - 2 * K) + 9 * K
    assert line["ms_per_step"] == pytest.approx(line["config"]["pivots_timed"] / line["value"] * 1e3 / 70)
