"""bench.py's plain run and --dump-outputs on the GPU.

A plain run (no --full) times the steps and prints the headline line with every sub-record null;
--dump-outputs DIR writes what the last timed step decoded as float32 / float64 .npy files.  Here the
file is small (C2 shape, 40,000 rows), so every array is written whole and is compared with the
oracle's decode of the same seeded file, element for element.  The sampling of larger arrays is
checked on the same shape with a small budget: the blocks come from the seeded positions of the
whole array, and a second dump writes the same files."""
import importlib.util
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, STEPS = 40_000, 3
# parquet physical type -> (dtype the decoded bytes are read as, dtype written)
TYPED = {1: (np.int32, np.float64), 2: (np.uint32, np.float64), 4: (np.float32, np.float32), 5: (np.float64, np.float64)}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
                        "--rows", str(ROWS), "--dump-outputs", str(out)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


def test_plain_line(plain_run):
    d, _ = plain_run
    assert d["full"] is False and d["steps"] == STEPS and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["metric"] and d["dtype"]
    assert d["ms_per_step"] > 0 and d["value"] > 0
    # value = decoded bytes of a step / the step's time
    assert abs(d["value"] - d["decoded_bytes_per_step"] / (d["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * d["value"] + 0.01
    assert d["config"]["rows_per_gpu"] == ROWS
    for k in ("kernels", "roofline", "launch", "e2e", "c3_strong", "mixed_1b", "c1_x10", "next_row", "cpu_baseline",
              "cpu_baseline_multicore", "cpu_comparator_pyarrow", "verified"):
        assert d[k] is None, k


def test_dumped_outputs_equal_the_oracle(plain_run, pq):
    _, out = plain_run
    data = pq.datasets.c2(rows=ROWS, seed=10)  # (bench.py's C2 file of rank 0)
    fr = O.FileReader(data)
    ncols = len(fr.columns)
    want = {}
    for rg in range(len(fr.row_groups)):
        for ci, col in enumerate(fr.columns):
            res = O.decode_chunk(fr.read_chunk(rg, ci))
            assert all(r.status == 0 for r in res)
            raw = np.frombuffer(b"".join(r.values for r in res), np.uint8)
            src, dst = TYPED.get(col.physical_type, (np.uint8, np.float32))
            want[f"rg{rg:03d}_c{ci:02d}_values"] = raw.view(src).astype(dst)
            if col.max_def > 0:
                want[f"rg{rg:03d}_c{ci:02d}_def_levels"] = np.concatenate([r.def_levels for r in res]).astype(np.float32)
    assert ncols == 6
    got = {p[:-4]: np.load(os.path.join(out, p)) for p in os.listdir(out)}
    assert sorted(got) == sorted(want)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    for name, w in want.items():
        g = got[name]
        assert g.dtype == w.dtype and g.dtype in (np.float32, np.float64), name
        assert np.array_equal(g, w), name


def test_sampled_dump_is_seeded_blocks_of_the_whole(pq, tmp_path):
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    native = pq.native
    data = pq.datasets.c2(rows=ROWS, seed=10)
    ctx = native.Context(0)
    f = native.File(data)
    ncols = len(f.columns())
    hb = f.load(0, 2, list(range(ncols)))
    b = native.Batch.from_host(ctx, hb)
    try:
        b.run()
        b.sync()
        chunks = hb.chunks()
        n_whole, _ = m.dump_outputs(ctx, b, chunks, ncols, 0, str(tmp_path / "whole"))
        m.DUMP_BUDGET, m.DUMP_BLOCK = n_whole * 2048, 64  # 2048 bytes an array: 256 or 512 elements
        for d in ("a", "b"):
            n, total = m.dump_outputs(ctx, b, chunks, ncols, 0, str(tmp_path / d))
            assert n == n_whole and total <= m.DUMP_BUDGET
    finally:
        b.close()
        hb.close()
        f.close()
        ctx.close()
    names = sorted(os.listdir(tmp_path / "whole"))
    assert names == sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) and len(names) == n_whole
    sampled = 0
    for name in names:
        whole, a = np.load(tmp_path / "whole" / name), np.load(tmp_path / "a" / name)
        assert np.array_equal(a, np.load(tmp_path / "b" / name)) and a.dtype == whole.dtype
        cap = 2048 // a.dtype.itemsize
        if len(whole) <= cap:
            assert np.array_equal(a, whole)
            continue
        sampled += 1
        rng = np.random.default_rng([m.DUMP_SEED, zlib.crc32(name[:-4].encode())])
        picks = np.sort(rng.choice(len(whole) // 64, size=cap // 64, replace=False))
        assert np.array_equal(a, np.concatenate([whole[p * 64:(p + 1) * 64] for p in picks])), name
    assert sampled >= ncols
