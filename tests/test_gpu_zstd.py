"""Device ZSTD (k_zstd, PQH_LOAD_DEVICE_ZSTD) against the oracle; mirrors test_gpu_codec.py.

* pqh_decompress_pages on its own: every stream of tests/zstd_blocks.py (pyarrow streams of five
  levels that use every feature of the format, hand-built frames, the cases where the reference
  differs from libzstd, seeded mutants) -- status and bytes must equal the expectations of
  test_zstd_codec.py (the oracle's libzstd; the reference where it differs), as the host route's do.
* one call holding SNAPPY, GZIP, ZSTD and plain-copy pages: each comes out right.
* whole pyarrow files (V1 / V2; flat, nullable, nested lists, dictionary fallback; 1 MiB pages of
  URL-like strings with multi-block frames) through decode_chunks, plain and staged, FileReader and
  RowGroupStream, chunk by chunk and row by row against the oracle.
* a corrupt page fails its chunk with PQH_ERR_DECOMPRESS exactly when the oracle rejects the block.
* default routing: barely compressible pages take the host route, the others the device's.
"""
import gzip
import io

import numpy as np
import pyarrow as pa
import pytest

import fixtures
import test_zstd_codec as TZ
import zstd_blocks as Z
from oracle import oracle as O
from parity import assert_chunk, oracle_chunk

pytestmark = pytest.mark.gpu

DECOMPRESS = 23


@pytest.fixture(scope="module")
def ctx(pq):
    return pq.native.Context(0)


@pytest.fixture(autouse=True)
def every_page_on_the_device(monkeypatch, request):
    if request.node.name.startswith("test_device_zstd_default_routing"):
        return
    monkeypatch.setenv("PQH_DEVICE_CODEC_MAX_RATIO", "0")


def _device_decompress(pq, ctx, blocks, sizes, codecs):
    """Every block as one codec page; returns [(status, bytes)]."""
    N = pq.native
    src, pages, soff, ioff = [], [], 0, 0
    for blk, size, codec in zip(blocks, sizes, codecs):
        pad = (-soff) % 64
        src.append(b"\0" * pad + blk)
        soff += pad
        ioff = (ioff + 63) & ~63
        pages.append(N.CodecPage(soff, ioff, len(blk), size, 0, codec, 0, 0))
        soff += len(blk)
        ioff += size
    s = np.frombuffer(b"".join(src) + b"\0" * N.PAYLOAD_PAD, np.uint8).copy()
    ds, dd = ctx.malloc(len(s)), ctx.malloc(ioff + N.PAYLOAD_PAD)
    try:
        ctx.h2d(ds, s.ctypes.data, len(s))
        st = ctx.decompress_pages(pages, ds, dd)
        img = ctx.d2h_array(dd, ioff) if ioff else np.zeros(0, np.uint8)
    finally:
        ctx.free(ds)
        ctx.free(dd)
    return [(st[i], img[p.image_offset:p.image_offset + p.image_len].tobytes()) for i, p in enumerate(pages)]


def _check(pq, ctx, cases):
    """cases: (name, stream, size, status, bytes) as test_zstd_codec.expected_cases gives them."""
    got = _device_decompress(pq, ctx, [c[1] for c in cases], [c[2] for c in cases], [O.ZSTD] * len(cases))
    ok = bad = 0
    for (name, s, size, est, eraw), (st, raw) in zip(cases, got):
        assert st == est, f"{name}: device status {st} vs expected {est}"
        if est == 0:
            assert raw == eraw, f"{name}: bytes differ"
        ok += est == 0
        bad += est != 0
    return ok, bad


def test_zstd_valid_streams(pq, ctx):
    cases = TZ.expected_cases()["valid"]
    assert len(cases) >= 65
    assert _check(pq, ctx, cases) == (len(cases), 0)


def test_zstd_hand_built_frames(pq, ctx):
    ok, bad = _check(pq, ctx, TZ.expected_cases()["hand"])
    assert ok >= 20 and bad >= 15, (ok, bad)


def test_zstd_follows_the_reference_where_libzstd_differs(pq, ctx):
    cases = TZ.expected_cases()["reference"]
    ok, bad = _check(pq, ctx, cases)
    assert ok == sum(1 for c in cases if c[3] == 0) and bad == sum(1 for c in cases if c[3])


def test_zstd_mutants(pq, ctx):
    cases = TZ.expected_cases()["mutants"]
    assert len(cases) >= 234
    ok, bad = _check(pq, ctx, cases)
    assert ok >= 40 and bad >= 80, (ok, bad)


def test_mixed_codecs_in_one_call(pq, ctx):
    """SNAPPY, GZIP, ZSTD and plain-copy pages interleaved in one pqh_decompress_pages call: every
    kernel leaves the other kernels' pages alone."""
    rng = np.random.default_rng(23)
    raws = [Z.url_lines(3000, 1), np.repeat(rng.integers(0, 1 << 40, 4000), 8).tobytes(),
            rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), b"", b"abc" * 50000]
    blocks, sizes, codecs = [], [], []
    for r in raws:
        for codec, blk in ((O.SNAPPY, pa.compress(r, codec="snappy", asbytes=True)), (O.GZIP, gzip.compress(r)),
                           (O.ZSTD, pa.compress(r, codec="zstd", asbytes=True)), (O.UNCOMPRESSED, r)):
            blocks.append(blk)
            sizes.append(len(r))
            codecs.append(codec)
    got = _device_decompress(pq, ctx, blocks, sizes, codecs)
    for i, (st, raw) in enumerate(got):
        assert st == 0 and raw == raws[i // 4], f"page {i} (codec {codecs[i]}): status {st}"


def _pyarrow_write(tbl, **kw):
    import pyarrow.parquet as pqa

    buf = io.BytesIO()
    pqa.write_table(tbl, buf, compression="ZSTD", **kw)
    return buf.getvalue()


_URL_FILE = {}


def url_file():
    """200,000 URL-like strings in 1 MiB pages (multi-block frames with repeat modes), and the
    oracle's decode of its chunks, made once."""
    if not _URL_FILE:
        urls = [b"https://www.example.com/news-%d/item%d?id=%d" % (i % 40, i % 500, i) for i in range(200_000)]
        data = _pyarrow_write(pa.table({"u": pa.array(urls, pa.binary())}), data_page_size=1 << 20, compression_level=3,
                              use_dictionary=False, row_group_size=100_000)
        fr = O.FileReader(data)
        expect = []
        for rg in range(len(fr.row_groups)):
            e = oracle_chunk(fr, rg, 0)
            e.routed = False
            expect.append(e)
        _URL_FILE.update(data=data, expect=expect)
    return _URL_FILE["data"], _URL_FILE["expect"]


def _files():
    yield "pyarrow-v1", fixtures.pyarrow_file(n=20000, version="1.0", compression="ZSTD")
    yield "pyarrow-v2", fixtures.pyarrow_file(n=20000, version="2.0", compression="ZSTD")
    yield "urls-1mib", url_file()[0]


@pytest.mark.parametrize("staged", [False, True])
def test_device_zstd_files(pq, ctx, staged):
    checked = zs = 0
    for name, data in _files():
        f = pq.native.File(data)
        ncols = len(f.columns())
        hb = f.load(0, f.num_row_groups, list(range(ncols)), device_zstd=True)
        zs += sum(c.codec == O.ZSTD for c in hb.codec_pages())
        hb.close()
        res = pq.reader.decode_chunks(ctx, f, 0, f.num_row_groups, list(range(ncols)), device_zstd=True,
                                      staged_runs=2 if staged else 0)
        fr = O.FileReader(data)
        for k, col in enumerate(res):
            rg, ci = divmod(k, ncols)
            exp = oracle_chunk(fr, rg, ci)
            exp.routed = False  # decoded here, not handed back
            assert col.status != pq.native.NOT_IMPLEMENTED, f"{name} rg{rg} {col.path}: NOT_IMPLEMENTED"
            assert_chunk(col, exp, where=f"{name} rg{rg} {col.path}")
            checked += 1
        f.close()
    assert checked > 30 and zs > 50, (checked, zs)


def test_file_reader_and_stream_with_device_zstd(pq, ctx):
    """The other public entry points: FileReader.ReadColumns / NextRow and RowGroupStream with the
    ZSTD keywords equal the oracle; without them the reader still raises UnsupportedCodecError.
    (On pyarrow's V1 file: its V2 ZSTD file stores some values sections uncompressed, which the
    reference's reader fails -- page_v2.go:125 decompresses them regardless -- so that file has no
    rows to compare; its chunks' errors are compared through the stream below and in
    test_device_zstd_files.)"""
    from test_records import _norm, oracle_rows

    data = fixtures.pyarrow_file(n=20000, version="1.0", compression="ZSTD")
    ofr = O.FileReader(data)
    ncols = len(ofr.columns)

    def expect(rg, ci):
        e = oracle_chunk(ofr, rg, ci)
        e.routed = False
        return e

    fr = pq.reader.FileReader(data, ctx=ctx, zstd=True, device_zstd=True)
    for rg in range(fr.RowGroupCount()):
        cols = fr.ReadColumns()
        assert len(cols) == ncols
        for ci, path in enumerate(fr.Columns()):
            assert_chunk(cols[path], expect(rg, ci), where=f"ReadColumns rg{rg} {path}")
        fr.SkipRowGroup()
    fr.close()
    with pytest.raises(pq.reader.UnsupportedCodecError):
        pq.reader.FileReader(data, ctx=ctx).ReadColumns()
    # rows: a smaller file of the same shape (the assembly is host Python)
    small = fixtures.pyarrow_file(n=1500, version="1.0", compression="ZSTD")
    want = oracle_rows(small)
    fr = pq.reader.FileReader(small, ctx=ctx, zstd=True, device_zstd=True)
    got = []
    while True:
        try:
            got.append(fr.NextRow())
        except EOFError:
            break
    fr.close()
    assert len(got) == len(want) == 1500
    for i, (g, w) in enumerate(zip(got, want)):
        assert _norm(g) == _norm(w), f"row {i}"
    for version in ("1.0", "2.0"):
        data = fixtures.pyarrow_file(n=20000, version=version, compression="ZSTD")
        ofr = O.FileReader(data)
        f = pq.native.File(data)
        st = pq.reader.RowGroupStream(f, list(range(ncols)), per_range=1, slots=2, device_zstd=True)
        try:
            seen = 0
            for a, b, batch, hb in st:
                for k, col in enumerate(st.column_data(batch, hb)):
                    assert_chunk(col, expect(a + k // ncols, k % ncols), where=f"stream {version} rg{a} {col.path}")
                    seen += 1
            assert seen == f.num_row_groups * ncols
        finally:
            st.close()
            f.close()


# (most flips land in raw literal bytes, which no decoder can notice: of seeds 0..59 the oracle rejects
# at least 4 of the 12 trials for 9, 10, 34, 35 and 58 only; 10 rejects 6.  None of these trials makes a
# stream that libzstd accepts and the reference rejects, test_zstd_codec.LIBZSTD_LENIENT_HUFFMAN_END.)
CORRUPT_SEED = 10


def corrupt_two_chunk_file():
    rng = np.random.default_rng(3)
    vals = np.repeat(rng.integers(0, 1 << 40, 3000), 8)
    return _pyarrow_write(pa.table({"v": pa.array(vals), "w": pa.array(vals[::-1].copy())}), data_page_size=8 * 1024,
                          use_dictionary=False)


def test_device_zstd_corrupt_page_fails_its_chunk(pq, ctx):
    """A bit flipped in a compressed ZSTD page: its chunk reports DECOMPRESS on the device exactly
    when the oracle rejects the block; the other chunk decodes."""
    data = corrupt_two_chunk_file()
    rng = np.random.default_rng(CORRUPT_SEED)
    f = pq.native.File(data)
    failed = ok = 0
    for trial in range(12):
        hb = f.load(0, 1, [0, 1], device_zstd=True)
        cps = hb.codec_pages()
        src = hb.payload()
        victim = cps[int(rng.integers(0, len(cps)))]
        assert victim.codec == O.ZSTD
        lo = victim.src_offset + victim.raw_len
        i = int(rng.integers(lo + 6, victim.src_offset + victim.src_len))  # (past the frame header descriptor)
        src[i] ^= 1 << int(rng.integers(0, 8))
        blk = bytes(src[lo:victim.src_offset + victim.src_len])
        st, _ = TZ.oracle_expected(blk, victim.image_len - victim.raw_len)
        b = pq.native.Batch.from_host(ctx, hb)
        b.run()
        b.sync()
        out = b.chunk_out(victim.chunk)
        if st:
            assert out.status == DECOMPRESS, f"trial {trial}: device status {out.status}"
            failed += 1
        else:
            assert out.status == 0, f"trial {trial}: device status {out.status}, the oracle accepts"
            ok += 1
        assert b.chunk_out(1 - victim.chunk).status == 0
        b.close()
        hb.close()
    f.close()
    assert failed >= 4, (failed, ok)


def test_device_zstd_url_pages_repeat(pq, ctx):
    """The 1 MiB-page file decoded with device ZSTD in plain and staged batches, three runs back to
    back each; every run equals the oracle's decode bit for bit."""
    data, expect = url_file()
    f = pq.native.File(data)
    for staged in (False, True):
        hb = f.load(0, f.num_row_groups, [0], ctx=ctx if staged else None, device_zstd=True)
        assert all(c.codec == O.ZSTD for c in hb.codec_pages())
        assert max(c.image_len for c in hb.codec_pages()) > 3 * 128 * 1024  # several blocks per page
        b = pq.native.Batch.staged(ctx, hb) if staged else pq.native.Batch.from_host(ctx, hb)
        for run in range(3):
            for _ in range(2):  # back to back, no sync in between
                b.run_staged() if staged else b.run()
            b.sync()
            res = b.page_results(hb.num_pages)
            pages = hb.pages()
            path, pt, tl, md, mr = f.columns()[0]
            for rg, ch in enumerate(hb.chunks()):
                span = range(ch.first_page, ch.first_page + ch.num_pages)
                info = [(pages[p].page_type, pages[p].num_values, res[p]) for p in span]
                col = pq.reader.ColumnData(path, (pt, tl, md, mr), b.chunk_out(rg), [res[p] for p in span], ctx, None, info)
                assert_chunk(col, expect[rg], where=f"staged={staged} run {run} rg{rg}")
        b.close()
        hb.close()
    f.close()


def test_device_zstd_default_routing(pq, ctx):
    """With device_zstd and the default PQH_DEVICE_CODEC_MAX_RATIO, pages of random values (ZSTD stores
    them in raw blocks) take the host route and arrive as plain copies, URL pages travel compressed;
    both equal the oracle."""
    rng = np.random.default_rng(11)
    n = 6000
    urls = [b"https://www.example.com/news-%d/item%d?id=%d" % (i % 40, i % 500, i) for i in range(n)]
    tbl = pa.table({"r": pa.array(rng.integers(-2**63, 2**63 - 1, n)), "u": pa.array(urls, pa.binary())})
    data = _pyarrow_write(tbl, data_page_size=16 * 1024, use_dictionary=False, row_group_size=3000)
    f = pq.native.File(data)
    hb = f.load(0, f.num_row_groups, [0, 1], device_zstd=True)
    kinds = {}
    for cp in hb.codec_pages():
        kinds.setdefault(cp.chunk % 2, set()).add(cp.codec)
    assert kinds[0] == {0} and kinds[1] == {O.ZSTD}, kinds
    hb.close()
    res = pq.reader.decode_chunks(ctx, f, 0, f.num_row_groups, [0, 1], device_zstd=True)
    fr = O.FileReader(data)
    for k, col in enumerate(res):
        exp = oracle_chunk(fr, *divmod(k, 2))
        exp.routed = False
        assert_chunk(col, exp, where=f"chunk {k}")
    f.close()
