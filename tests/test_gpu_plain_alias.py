"""Required fixed-width PLAIN chunks handed out in place (pqh_chunk_out.values pointing into the
batch's payload, no copy tiles): which chunks take the path, that every result is what the copy
path (PQH_PLAIN_ALIAS=0) and the oracle give, and that nothing writes through the pointer."""
import numpy as np
import pytest

import fixtures
import pqcraft
from oracle import oracle as O
from parity import Expected, assert_chunk, oracle_chunk

pytestmark = pytest.mark.gpu

PACKED = {"i64_plain", "flba16"}
I64 = (2, 0, 0, 0)  # (physical type INT64, type_length, max_def, max_rep)


@pytest.fixture(scope="module")
def ctx(pq):
    return pq.native.Context(0)


def _snapshot(col):
    """Everything a chunk reports, as comparable host data."""
    arr = lambda a: None if a is None else np.asarray(a).view(np.uint8).tobytes()  # noqa: E731
    pages = [(r.status, r.phase, r.index, r.num_non_null, r.num_nil, r.value_offset, r.level_offset) for r in col.pages]
    return (col.status, col.error_page, col.error_phase, col.error_index, col.num_values, col.num_non_null,
            arr(col.values), arr(col.offsets), arr(col.data), arr(col.def_levels), arr(col.rep_levels),
            arr(col.value_nil), pages)


def _decode_file(pq, data, alias, monkeypatch):
    """Decode every chunk in a context of its own (the switch is read when a batch is created)."""
    monkeypatch.setenv("PQH_PLAIN_ALIAS", "1" if alias else "0")
    ctx = pq.native.Context(0)
    f = pq.native.File(data)
    cols = list(range(len(f.columns())))
    res, b, hb = pq.reader.decode_chunks(ctx, f, 0, f.num_row_groups, cols, return_batch=True)
    paths = b.paths()
    b.close()
    hb.close()
    ctx.close()
    return f, res, paths


@pytest.mark.parametrize("v2", [False, True])
def test_default_against_copy_path(pq, monkeypatch, v2):
    data = fixtures.flat_all_types(n=6000, v2=v2, page=16 * 1024, rows_per_group=3000)
    f, on, paths_on = _decode_file(pq, data, True, monkeypatch)
    _, off, paths_off = _decode_file(pq, data, False, monkeypatch)
    ncols = len(f.columns())
    fr = O.FileReader(data)
    assert len(on) == len(off) == ncols * f.num_row_groups
    for k, (a, b) in enumerate(zip(on, off)):
        rg, ci = divmod(k, ncols)
        assert _snapshot(a) == _snapshot(b), f"rg{rg} {a.path}: in place and copied results differ"
        assert_chunk(a, oracle_chunk(fr, rg, ci), where=f"rg{rg} {a.path}")
    eligible = sum(1 for c in on if c.path in PACKED)
    assert eligible == 2 * f.num_row_groups
    assert paths_on["plain_alias_chunks"] == eligible and paths_off["plain_alias_chunks"] == 0


def _int64_pages(seed=3, counts=(1000, 1001, 7)):
    rng = np.random.default_rng(seed)
    return [rng.integers(-2**62, 2**62, n).astype("<i8").tobytes() for n in counts]


def _hand_batch(pq, ctx, images, counts, base=0, gap_before=None, col=I64, runs=2, ptype=O.DATA_PAGE):
    """One chunk of PLAIN pages laid out by hand in a ctx.malloc payload: page i holds images[i] and
    announces counts[i] values; the first image starts at `base`, `gap_before` = (page, bytes) leaves
    a hole.  Runs the batch `runs` times with a sync after each; returns (ColumnData, chunk_out,
    paths, payload range, payload unchanged)."""
    N = pq.native
    off, pages, blob = base, [], bytearray(base)
    for i, (img, n) in enumerate(zip(images, counts)):
        if gap_before and gap_before[0] == i:
            blob += bytes(gap_before[1])
            off += gap_before[1]
        pages.append(N.Page(off, len(img), ptype, n, 0, 0, 0, 0, 0))
        blob += img
        off += len(img)
    arr = np.frombuffer(bytes(blob) + b"\0" * N.PAYLOAD_PAD, dtype=np.uint8).copy()
    d = ctx.malloc(len(arr))
    try:
        ctx.h2d(d, arr.ctypes.data, len(arr))
        ctx.sync()
        b = N.Batch.from_tables(ctx, [N.Chunk(N.Column(*col), 0, len(pages), 0, 0)], pages, d, off)
        for _ in range(runs):
            b.run()
            b.sync()
        o = b.chunk_out(0)
        cd = pq.reader.ColumnData("hand", col, o, b.page_results(len(pages)), ctx)
        paths = b.paths()
        same = np.array_equal(ctx.d2h_array(d, len(arr)), arr)
        vptr = o.values or 0
        b.close()
        return cd, vptr, paths, (d, d + off), same
    finally:
        ctx.free(d)


def _expect(images, counts, col=I64, ptype=O.DATA_PAGE):
    """The oracle's result of the chunk, page by page (readValues stops at the first failing page)."""
    e = Expected()
    vals = []
    for i, (img, n) in enumerate(zip(images, counts)):
        r = O.decode_page(col, ptype, n, 0, 0, 0, img, None)
        if r.status and e.status == 0:
            e.status, e.phase, e.index, e.page = r.status, r.phase, r.index, i
        e.nn += r.nn
        vals.append(r.values)
    e.values = b"".join(vals)
    return e


@pytest.mark.parametrize("flat,profile", [("1", False), ("0", False), ("0", True)])
def test_hand_laid_tables(pq, monkeypatch, flat, profile):
    """pqh_batch_create decides from the tables alone.  The aliased batch holds nothing but aliased
    chunks: k_flat with no tiles (PQH_FLAT=1), or k_prologue + k_scan and no k_expand launch, replayed
    from a captured graph or launched directly (profiled)."""
    monkeypatch.setenv("PQH_FLAT", flat)
    ctx = pq.native.Context(0, profile=profile)
    counts = (1000, 1001, 7)
    images = _int64_pages()
    want = _expect(images, counts)
    assert want.status == 0 and want.values == b"".join(images)
    for ptype in (O.DATA_PAGE, O.DATA_PAGE_V2):
        cd, vptr, paths, (lo, hi), same = _hand_batch(pq, ctx, images, counts, ptype=ptype)
        assert_chunk(cd, want, where="contiguous")
        assert paths["plain_alias_chunks"] == 1 and lo <= vptr < hi and vptr == lo
        assert same, "the payload changed under an aliased batch"
        assert [r.value_offset for r in cd.pages] == [0, 1000, 2001] and all(r.status == 0 for r in cd.pages)
    cd, vptr, paths, (lo, hi), same = _hand_batch(pq, ctx, images, counts, gap_before=(1, 8))
    assert_chunk(cd, want, where="gap before the second page")
    assert paths["plain_alias_chunks"] == 0 and not (lo <= vptr < hi) and same
    cd, vptr, paths, (lo, hi), same = _hand_batch(pq, ctx, images, counts, base=8)
    assert_chunk(cd, want, where="base offset by 8")
    assert paths["plain_alias_chunks"] == 0 and not (lo <= vptr < hi) and same
    cd, vptr, paths, (lo, hi), same = _hand_batch(pq, ctx, images, counts, base=128)
    assert_chunk(cd, want, where="base offset by 128")
    assert paths["plain_alias_chunks"] == 1 and vptr == lo + 128 and same
    ctx.close()


def test_never_aliased_pages(pq, ctx):
    counts = (1000, 1001, 7)
    images = _int64_pages(seed=5)
    # 8 bytes short: the page's last value cannot be read -- the reference's error, at its page and index
    short = [images[0], images[1][:-8], images[2]]
    want = _expect(short, counts)
    assert pq.native.STATUS[want.status] in ("EOF", "UNEXPECTED_EOF") and want.page == 1
    cd, vptr, paths, (lo, hi), same = _hand_batch(pq, ctx, short, counts)
    assert paths["plain_alias_chunks"] == 0 and same
    assert_chunk(cd, want, where="short page")
    assert cd.error_page == 1
    # 8 bytes too many: the trailing bytes are not values
    long_ = [images[0], images[1] + b"\xaa" * 8, images[2]]
    want = _expect(long_, counts)
    assert want.status == 0 and want.values == b"".join(images)
    cd, vptr, paths, (lo, hi), same = _hand_batch(pq, ctx, long_, counts)
    assert paths["plain_alias_chunks"] == 0 and not (lo <= vptr < hi) and same
    assert_chunk(cd, want, where="long page")


def _file_unaliased(pq, ctx, data, expect_pages=None):
    f = pq.native.File(data)
    ncols = len(f.columns())
    res, b, hb = pq.reader.decode_chunks(ctx, f, 0, f.num_row_groups, list(range(ncols)), return_batch=True)
    assert b.paths()["plain_alias_chunks"] == 0
    if expect_pages is not None:
        expect_pages(hb.pages())
    fr = O.FileReader(data)
    for k, col in enumerate(res):
        rg, ci = divmod(k, ncols)
        assert_chunk(col, oracle_chunk(fr, rg, ci), where=f"rg{rg} {col.path}")
    b.close()
    hb.close()
    return res


def test_never_aliased_chunks(pq, ctx):
    W = fixtures.W
    rng = np.random.default_rng(17)
    n = 6000

    def fallback(pages):  # dictionary pages, then PLAIN pages, in one chunk
        assert pages[0].page_type == O.DICTIONARY_PAGE
        encs = {p.encoding for p in pages[1:]}
        assert W.PLAIN in encs and len(encs) == 2, encs

    _file_unaliased(pq, ctx, W.flat([("d", W.Column(W.INT64, rng.integers(-2**62, 2**62, n), dict_page_limit=4096),
                                       W.REQUIRED)], n, max_page_size=8 * 1024), fallback)
    _file_unaliased(pq, ctx, W.flat([("o", W.optional(W.DOUBLE, rng.normal(size=n), rng.random(n) < 0.1, use_dict=False),
                                       W.OPTIONAL)], n, v2=True, max_page_size=8 * 1024))
    # PLAIN INT96 whose last value is short: the reference's nil slot
    blk = rng.integers(0, 256, 12 * 99 + 5, dtype=np.uint8).tobytes()
    res = _file_unaliased(pq, ctx, pqcraft.int96_file([(None, [(blk, 100, 0, None, None)])]))
    assert res[0].value_nil is not None and int(res[0].value_nil.sum()) == 1


def test_staged_and_streaming(pq, ctx):
    data = fixtures.flat_c2_like()
    f = pq.native.File(data)
    ncols = len(f.columns())
    cols = list(range(ncols))
    fr = O.FileReader(data)
    want = [oracle_chunk(fr, rg, ci) for rg in range(f.num_row_groups) for ci in range(ncols)]
    hb = f.load(0, f.num_row_groups, cols, ctx=ctx)
    b = pq.native.Batch.staged(ctx, hb)
    for _ in range(2):
        b.run_staged()
        b.sync()
    assert b.paths()["plain_alias_chunks"] == 2 * f.num_row_groups
    for k, col in enumerate(pq.reader.batch_columns(ctx, f, b, hb, cols)):
        assert_chunk(col, want[k], where=f"staged chunk {k} {col.path}")
    b.close()
    hb.close()
    st = pq.reader.RowGroupStream(f, cols, per_range=1, slots=2)
    try:
        seen = 0
        for a, e, batch, shb in st:
            assert batch.paths()["plain_alias_chunks"] == 2 * (e - a)
            for k, col in enumerate(st.column_data(batch, shb)):
                assert_chunk(col, want[a * ncols + k], where=f"stream rg{a} chunk {k} {col.path}")
            seen += e - a
        assert seen == f.num_row_groups
    finally:
        st.close()
        f.close()


def test_small_batch_one_launch(pq, ctx):
    """A small C2-shaped batch stays on k_flat's one launch (as before: its chunks are flat, required or
    nullable with V2 pages), now with no copy tiles for the two aliased chunks."""
    data = fixtures.flat_c2_like(n=4000)
    f = pq.native.File(data)
    res, b, hb = pq.reader.decode_chunks(ctx, f, 0, f.num_row_groups, list(range(6)), return_batch=True)
    paths = b.paths()
    assert paths["flat_active"] == 1 and paths["flat_fallbacks"] == 0, paths
    assert paths["plain_alias_chunks"] == 2 * f.num_row_groups
    fr = O.FileReader(data)
    for k, col in enumerate(res):
        rg, ci = divmod(k, 6)
        assert_chunk(col, oracle_chunk(fr, rg, ci), where=f"rg{rg} {col.path}")
    b.close()
    hb.close()
