"""The host walker's packed layout (pqh_file_load, no GPU): a required, non-repeated, fixed-width
chunk of PLAIN data pages only has its page images placed back to back -- the payload then already
holds the chunk's values array, which the batch hands out in place (pqh_chunk_out.values) -- while
every other chunk keeps 64-byte aligned pages.  Images are compared with the oracle's walker page by
page; gaps and the pad must be zero."""
import numpy as np
import pytest

import fixtures
import pqcraft
from oracle import oracle as O

PACKED = {"i64_plain", "flba16"}


def _walk(pq, data):
    f = pq.native.File(data)
    cols = f.columns()
    hb = f.load(0, f.num_row_groups, list(range(len(cols))))
    return f, cols, hb


def _check_layout(pq, data, packed_paths):
    """Every chunk's layout and images; returns {path: [pages per chunk]} of the packed chunks."""
    f, cols, hb = _walk(pq, data)
    fr = O.FileReader(data)
    pages, payload = hb.pages(), hb.payload()
    assert len(payload) == hb.payload_bytes + pq.native.PAYLOAD_PAD
    covered = np.zeros(len(payload), bool)
    packed = {}
    for k, ch in enumerate(hb.chunks()):
        rg, ci = divmod(k, len(cols))
        path = cols[ci][0]
        och = fr.read_chunk(rg, ci)
        assert ch.host_status == och.status == 0, (path, ch.host_status, och.status)
        span = [pages[p] for p in range(ch.first_page, ch.first_page + ch.num_pages)]
        dpages = [p for p in span if p.page_type != O.DICTIONARY_PAGE]
        assert len(dpages) == len(och.pages), path
        for p, op in zip(dpages, och.pages):
            assert (p.page_type, p.num_values, p.encoding) == (op.page_type, op.num_values, op.encoding), path
            assert payload[p.image_offset:p.image_offset + p.image_len].tobytes() == op.image, (path, rg)
        for p in span:
            assert 0 <= p.image_offset and p.image_offset + p.image_len <= hb.payload_bytes, path
            assert not covered[p.image_offset:p.image_offset + p.image_len].any(), f"{path}: images overlap"
            covered[p.image_offset:p.image_offset + p.image_len] = True
        assert span[0].image_offset % 64 == 0, path
        if path in packed_paths:
            assert len(dpages) == len(span), path
            for a, b in zip(span, span[1:]):
                assert b.image_offset == a.image_offset + a.image_len, f"{path} rg{rg}: pages not back to back"
            packed.setdefault(path, []).append(len(span))
        else:
            assert all(p.image_offset % 64 == 0 for p in span), f"{path} rg{rg}: a page is not 64-aligned"
    assert not payload[~covered].any(), "bytes between the areas (or the pad) are not zero"
    hb.close()
    f.close()
    return packed


@pytest.mark.parametrize("v2", [False, True])
@pytest.mark.parametrize("codec", [O.UNCOMPRESSED, O.SNAPPY])
def test_packed_and_aligned_chunks(pq, v2, codec):
    data = fixtures.flat_all_types(n=6000, v2=v2, codec=codec, page=16 * 1024, rows_per_group=3000)
    packed = _check_layout(pq, data, PACKED)
    assert set(packed) == PACKED
    # several pages per chunk (their 16 KiB pages are multiples of 64 bytes: test_packed_flba3_and_int32
    # has the pages that packing moves off the 64-byte grid)
    assert all(n >= 2 for counts in packed.values() for n in counts), packed


def test_packed_flba3_and_int32(pq):
    """Value sizes 3 and 4 with odd values per page and an odd number of pages: page images start at
    offsets that are no multiple of the value size's alignment, let alone 64."""
    W = fixtures.W
    rng = np.random.default_rng(41)
    n = 5001
    fl3 = W.flat([("f3", W.Column(W.FIXED_LEN_BYTE_ARRAY, rng.integers(0, 256, (n, 3), dtype=np.uint8), type_length=3,
                                  use_dict=False), W.REQUIRED)], n, max_page_size=1000)
    i32 = W.flat([("i", W.Column(W.INT32, rng.integers(-2**31, 2**31 - 1, n).astype(np.int32), use_dict=False),
                   W.REQUIRED)], n, v2=True, max_page_size=1100)
    for data, path in ((fl3, "f3"), (i32, "i")):
        packed = _check_layout(pq, data, {path})
        assert len(packed[path]) == 1 and packed[path][0] >= 3, packed
        f, cols, hb = _walk(pq, data)
        assert any(p.image_offset % 4 for p in hb.pages()) or path == "i"
        assert any(p.image_offset % 64 for p in hb.pages()), "no page moved: the case checks nothing"
        assert sum(p.num_values for p in hb.pages()) == n
        hb.close()


def test_device_codec_load_keeps_aligned_pages(pq, monkeypatch):
    """A device-codec load keeps every image 64-aligned (its images are rebuilt on the device), also for
    the chunks a plain load packs."""
    monkeypatch.setenv("PQH_DEVICE_CODEC_MAX_RATIO", "0")
    data = fixtures.flat_all_types(n=6000, v2=True, codec=O.SNAPPY, page=16 * 1024, rows_per_group=3000)
    f = pq.native.File(data)
    hb = f.load(0, f.num_row_groups, list(range(len(f.columns()))), device_snappy=True)
    assert hb.codec_pages() and all(p.image_offset % 64 == 0 for p in hb.pages())
    hb.close()


def test_truncated_last_page_is_not_packed(pq):
    """A chunk whose last page ends past the end of the file (its header and the chunk metadata still
    announce the full page): the walk fails there as the oracle's does, and the pages listed before
    it keep their 64-aligned places."""
    vals = [np.arange(k, k + n, dtype=np.int32).tobytes() for k, n in ((0, 333), (1000, 335), (2000, 501))]
    whole = pqcraft.file_with_blocks([[(v, len(v), len(v) // 4) for v in vals]], O.UNCOMPRESSED)
    assert _check_layout(pq, whole, {"v"}) == {"v": [3]}
    flen = int(np.frombuffer(whole[-8:-4], "<i4")[0])
    body, footer = whole[:-(8 + flen)], whole[-(8 + flen):]
    cut = len(footer) + 200  # more than the footer: the last page's block reaches past the file's end
    assert cut < len(vals[2])
    data = body[:-cut] + footer
    och = O.FileReader(data).read_chunk(0, 0)
    assert och.status == O.ERR_DECOMPRESS and len(och.pages) == 2
    f, cols, hb = _walk(pq, data)
    ch, pages, payload = hb.chunks()[0], hb.pages(), hb.payload()
    assert ch.host_status == och.status and ch.num_pages == 2 and len(pages) == 2
    for p, op in zip(pages, och.pages):
        assert p.image_offset % 64 == 0
        assert payload[p.image_offset:p.image_offset + p.image_len].tobytes() == op.image
    assert pages[1].image_offset != pages[0].image_offset + pages[0].image_len
    hb.close()
