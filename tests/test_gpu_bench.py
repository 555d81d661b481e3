"""bench.py's plain run -- `bench.py --gpus 1 --steps K --warmup W` times the K steps and nothing else -- and what
--dump-outputs writes: the last timed step's top-k list, the same from run to run and the same as that query's search."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import nifs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, DIM, STEPS, WARMUP = 100000, 64, 7, 2


def plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--rows", str(ROWS), "--dim", str(DIM), "--release-wait", "0", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_a_plain_run_times_its_steps_and_dumps_the_last_ones_hits(tmp_path, nifs):
    import torch
    import bench
    line = plain_run(tmp_path / "a")
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["unit"] == "queries/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    assert not {"roofline", "long_run", "side", "cpu_baseline", "summary"} & set(line), sorted(line)
    ids, scores = np.load(tmp_path / "a" / "hit_ids.npy"), np.load(tmp_path / "a" / "hit_scores.npy")
    assert ids.dtype == np.float64 and scores.dtype == np.float32 and len(ids) == len(scores) == 10
    plain_run(tmp_path / "b")
    for name in ("hit_ids.npy", "hit_scores.npy"):
        assert np.load(tmp_path / "a" / name).tobytes() == np.load(tmp_path / "b" / name).tobytes(), name

    # the same corpus and the last timed query, searched here
    x = bench.build_shard(torch, torch.device("cuda", 0), ROWS, DIM, bench.SEED_CORPUS)
    ref = nifs._flat_new(nifs.METRIC_CODE["cosine"])
    nifs.flat_set_reduce_order(ref, bench.ORDER_CODE["sse2"])
    assert nifs.flat_load_device_matrix(ref, bench.doc_ids(0, ROWS), x.data_ptr(), ROWS, DIM) == ("ok", ())
    del x
    q = bench.normalized_queries(WARMUP + STEPS, DIM, bench.SEED_QUERY)[WARMUP + STEPS - 1]
    status, hits = nifs.flat_search(ref, q, 10)
    assert status == "ok"
    assert [b"doc-%d" % v for v in ids.astype(np.int64)] == [h[0] for h in hits]
    assert scores.tobytes() == np.array([h[1] for h in hits], dtype=np.float32).tobytes()
