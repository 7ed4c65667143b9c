"""bench.py --dump-outputs: what the timed path computed in its last step, as float64 .npy files, exact and comparable between
builds (a fixed sample of the superclusters, at most 64 MB); and a plain run that prints the headline alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle_lib as O
from vcfdist_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALAR_FIELDS = ("sc_phase", "orig_phase_dist", "swap_phase_dist")
ALN_FIELDS = ("aln_dist", "aln_end_plane", "aln_beg_plane", "aln_status")


def check_dump(d, res, batch, counts):
    """every dumped array is finite and equals `res` / `counts` on the sampled superclusters, bit for bit (a float field through
    its value where finite and <name>_nonfinite where not)"""
    assert all(np.isfinite(np.load(os.path.join(d, f))).all() for f in os.listdir(d))
    idx = np.load(os.path.join(d, "sc_index.npy"))
    assert idx.dtype == np.float64 and np.array_equal(idx, np.unique(idx)) and len(idx) > 0
    idx = idx.astype(np.int64)
    for name in ALN_FIELDS:
        got = np.load(os.path.join(d, name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, getattr(res, name).reshape(-1, 4)[idx].ravel().astype(np.float64)), name
    for name in SCALAR_FIELDS:
        assert np.array_equal(np.load(os.path.join(d, name + ".npy")), getattr(res, name)[idx].astype(np.float64)), name
    var_idx = [np.concatenate([np.arange(batch.var_off[h][i], batch.var_off[h][i + 1]) for i in idx]).astype(np.int64) for h in range(4)]
    for name, dt in res.PER_VAR:
        got = np.load(os.path.join(d, name + ".npy"))
        want = np.concatenate([getattr(res, name)[h][w][var_idx[h]] for h in range(4) for w in range(2)])
        if dt == np.float32:
            code = np.load(os.path.join(d, name + "_nonfinite.npy"))
            assert np.array_equal(code, np.select([np.isnan(want), np.isposinf(want), np.isneginf(want)], [1, 2, 3], 0)), name
            fin = code == 0
            assert np.array_equal(got[fin].astype(np.float32).view(np.uint32), want[fin].view(np.uint32)) and not got[~fin].any(), name
        else:
            assert np.array_equal(got, want.astype(np.float64)), name
    assert np.array_equal(np.load(os.path.join(d, "counts.npy")), counts.astype(np.float64))
    return idx


def test_dump_outputs_is_exact_sampled_and_bounded(tmp_path, monkeypatch):
    syn = api.Synth(n_sc=2000, len_a=8, len_b=300, len_max=300, seed=11, var_per_base=0.03)
    batch = syn.batch()
    res = O.run(batch)
    res.credit[0][0][:3] = [np.nan, np.inf, -np.inf]        # (credit is 1 - query_ed / ref_ed: NaN at 0 / 0, -inf where ref_ed is 0)
    counts = np.arange(2 * 4 * 3 * 61, dtype=np.int64).reshape(2, 4, 3, 61)
    bench.dump_outputs(str(tmp_path / "all"), res, counts, batch)
    assert len(check_dump(str(tmp_path / "all"), res, batch, counts)) == batch.n_sc       # small enough: every supercluster
    assert np.load(str(tmp_path / "all" / "credit_nonfinite.npy"))[:3].tolist() == [1, 2, 3]
    monkeypatch.setattr(bench, "DUMP_BYTES", 100_000)
    for k in ("a", "b"):
        bench.dump_outputs(str(tmp_path / k), res, counts, batch)
    ia, ib = (check_dump(str(tmp_path / k), res, batch, counts) for k in ("a", "b"))
    assert 0 < len(ia) < batch.n_sc and np.array_equal(ia, ib)                          # a fixed sample
    data = sum(np.load(str(tmp_path / "a" / f)).nbytes for f in os.listdir(tmp_path / "a") if f != "counts.npy")
    assert data <= 100_000


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_steps_results(tmp_path):
    """a plain run (one batch in flight, so the last step's batch is the one of --seed) prints the headline alone, and its dump
    is the CPU oracle's result on that batch"""
    d = str(tmp_path / "out")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n-sc", "3000", "--steps", "3", "--warmup", "1",
                          "--in-flight", "1", "--dump-outputs", d], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == "supercluster-alignments/sec" and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert not {"roofline", "cpu_baseline", "one_pass", "one_at_a_time", "secondary", "summary"} & set(line)
    syn = bench.make_workload(api, 3000, 0x5eed, "wgs_synth")
    batch = syn.batch()
    want = O.run(batch)
    counts = O.oracle_pr_counts(O.lib(), batch.var_off, want, syn.var_class(), None)
    assert counts[:, 3].sum() > 0
    check_dump(d, want, batch, counts)
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64_000_000
