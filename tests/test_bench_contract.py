"""-m gpu: bench.py's one-line JSON contract at a reduced size (the driver runs it at full size): the keys the driver and
the judge read are there; under --full the full-size parity block is green and the host-fed leg and the CPU baseline report;
a plain run prints the headline alone and --dump-outputs writes the same result from run to run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--reads", "400000", "--steps", "1", "--warmup", "1",
                          "--cpu-sample-reads", "20000", "--host-fed-batches", "1", "--full"] + list(extra),
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_has_what_the_driver_reads():
    d = _run()
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["higher_is_better"] is True and d["unit"] == "Gbases/s"
    assert d["dtype"] == "int64" and d["data"] == "synthetic" and "workload" in d["config"] and d["vs_baseline"] is None
    assert d["value"] > 0 and d["ms_per_step"] > 0
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["measured_copy_gb_per_s"] and r["measured_copy_gb_per_s"] > 1000
    assert d["parity_fullsize"] is True and d["parity"]["ok"] is True
    assert d["parity"]["kmers_checked"] == d["config"]["kmers_per_gpu"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["all_cores"]["cores"] >= 1
    h = d["host_fed"]
    assert h["source"] == "pinned RAM" and h["gbases_per_s"] > 0 and h["h2d_gb_per_s"] > 0 and 0 <= h["overlap_frac"] <= 1


def test_bench_plain_run_prints_the_headline_alone_and_dumps_its_result(tmp_path):
    import numpy as np
    runs = []
    for name in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reads", "5000", "--steps", "2",
                              "--warmup", "1", "--dump-outputs", str(tmp_path / name)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "Gbases/s"
        assert d["higher_is_better"] is True and d["dtype"] == "int64" and d["metric"].startswith("Gbases/s FASTQ->k-mer count")
        # value is the bases of one step over ms_per_step; the line rounds ms_per_step to 0.01 ms and value to 1e-4
        assert abs(d["value"] - 5000 * 150 / (d["ms_per_step"] * 1e-3) / 1e9) <= d["value"] * 0.0051 / d["ms_per_step"] + 1e-4
        for moved in ("roofline", "kernels", "parity", "host_fed", "cpu_baseline", "extra"):
            assert moved not in d, moved
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["counts.npy", "keys.npy", "keys_hi.npy", "keys_lo.npy", "summary.npy"]
        runs.append((d, {f: np.load(tmp_path / name / f) for f in files}))
    (d, a), (_, b) = runs
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64_000_000
    n, total, n_reads, n_bases, n_kmers, n_bytes = (int(x) for x in a["summary.npy"])
    assert (n_reads, n_bases, n_kmers, n_bytes) == (5000, 5000 * 150, 5000 * 120, 5000 * 316)
    assert n == d["config"]["distinct_rank0"] == a["keys.npy"].size == a["counts.npy"].size
    assert total == n_kmers == int(a["counts.npy"].sum())
    keys = a["keys_hi.npy"].astype(np.int64) << 31 | a["keys_lo.npy"].astype(np.int64)
    assert np.all(np.diff(keys) > 0) and np.array_equal(keys.astype(np.float64), a["keys.npy"])
    for f in a:                                              # the same arguments: the same inputs, the same result
        assert np.array_equal(a[f], b[f]), f


def test_dump_outputs_samples_a_large_result_at_fixed_positions(tmp_path):
    """a result of more than DUMP_SAMPLE elements: DUMP_SAMPLE seeded positions, the first and the last among them"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from bionumpy_amd.device import HArray
    from bionumpy_amd.pipeline import BatchStats
    n = 3 * bench.DUMP_SAMPLE + 7
    keys = torch.arange(n, dtype=torch.int64, device="cuda") * ((1 << 62) // n) + 5          # (beyond 2^53: float64 rounds them)
    counts = torch.arange(n, dtype=torch.int64, device="cuda") % 11 + 1
    stats = BatchStats(1, 2, 3, 4)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), (HArray(dev=keys), HArray(dev=counts)), stats, 20260925, 0, 1)
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["counts.npy", "keys.npy", "keys_hi.npy", "keys_lo.npy", "positions.npy", "summary.npy"]
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64_000_000
    pos = a["positions.npy"].astype(np.int64)
    assert pos.size == bench.DUMP_SAMPLE and pos[0] == 0 and pos[-1] == n - 1 and np.all(np.diff(pos) >= 0)
    assert len(np.unique(pos)) > 0.8 * pos.size                                              # (drawn, not a prefix)
    want = keys.cpu().numpy()[pos]
    assert np.array_equal(a["keys_hi.npy"].astype(np.int64) << 31 | a["keys_lo.npy"].astype(np.int64), want)
    assert np.array_equal(a["keys.npy"], want.astype(np.float64)) and np.array_equal(a["counts.npy"], counts.cpu().numpy()[pos])
    assert a["summary.npy"].tolist() == [n, int(counts.sum().item()), 1, 2, 3, 4]
    for f in a:
        assert np.array_equal(a[f], np.load(tmp_path / "b" / f)), f


def test_bench_virtual_ranks_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--virtual-ranks", "4", "--reads", "400000", "--steps", "1",
                          "--warmup", "0"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert d["virtual_ranks"] == 4 and len(d["int64_words_received_per_rank"]) == 4 and d["plan"] == "keys"
    assert sum(d["int64_words_received_per_rank"]) == 400000 * 120


def test_bench_from_file_line(tmp_path):
    """--from-file: the reader's stream form over a FASTQ file it writes first; reads add up, checksums match"""
    path = str(tmp_path / "reads.fq")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--from-file", path, "--reads", "300000", "--steps", "1",
                          "--warmup", "1", "--file-chunk-mb", "32"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert d["reads_seen_by_all_ranks"] == 300000 and d["reads_add_up"] is True and d["parity_fullsize"] is True
    assert d["file_bytes"] == 300000 * 316 and d["gbases_per_s"] > 0
