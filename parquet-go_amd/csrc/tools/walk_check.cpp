// walk_check.cpp — stand-alone driver for the host page walker (host/file_reader.cpp pqh_file_load_ex
// over host/codec.cpp).  Opens the Parquet file named on the command line, walks every column of
// every row group with host codecs and with PQH_LOAD_DEVICE_SNAPPY, and checks the layout the walker
// promises: every page image (and, for a device-codec load, every page's source bytes) lies inside
// the payload, no two overlap, and a chunk the walker packs (a required, non-repeated, fixed-width
// chunk of PLAIN data pages: its images are its values array) is contiguous while every other page
// is 64-byte aligned.  Every payload byte is read, pad included, so a byte the walker left
// unwritten or a write past the buffer is a sanitizer report.  No HIP: meant to be built with
// -fsanitize=address,undefined and run by hand:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//       csrc/host/file_reader.cpp csrc/host/codec.cpp csrc/tools/walk_check.cpp -lz -lpthread \
//       -o walk_check && ./walk_check file.parquet
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../host/internal.h"

namespace pqhip {
// the pinned pool lives with the device side (host/batch.hip); pqh_file_load_ex never asks for it
std::shared_ptr<uint8_t> pinned_acquire(pqh_ctx*, size_t) { return nullptr; }
}  // namespace pqhip

static int check_load(pqh_file* f, uint32_t flags, const char* what) {
  const int32_t ncols = pqh_file_num_columns(f), nrg = pqh_file_num_row_groups(f);
  std::vector<int32_t> cols(static_cast<size_t>(ncols));
  for (int32_t i = 0; i < ncols; i++) cols[size_t(i)] = i;
  pqh_host_batch* hb = nullptr;
  const int rc = pqh_file_load_ex(f, 0, nrg, cols.data(), ncols, 1, flags, &hb);
  if (rc != PQH_OK) {
    printf("%s: load failed with %d (%s)\n", what, rc, pqh_file_error(f));
    return 1;
  }
  int bad = 0;
  const pqh_chunk* chunks = pqh_host_batch_chunks(hb);
  const pqh_page* pages = pqh_host_batch_pages(hb);
  const pqh_codec_page* cps = pqh_host_batch_codec_pages(hb);
  const int32_t nch = pqh_host_batch_num_chunks(hb), npg = pqh_host_batch_num_pages(hb);
  const int32_t ncp = pqh_host_batch_num_codec_pages(hb);
  const int64_t payload = pqh_host_batch_payload_bytes(hb);
  // the images' space: the payload (host codecs) or the image buffer the device rebuilds (device codecs)
  const int64_t image_space = ncp ? pqh_host_batch_image_bytes(hb) : payload;
  std::vector<std::pair<int64_t, int64_t>> spans, src_spans;
  int packed = 0;
  for (int32_t c = 0; c < nch; c++) {
    const pqh_chunk& C = chunks[c];
    if (C.first_page < 0 || C.num_pages < 0 || int64_t(C.first_page) + C.num_pages > npg) {
      printf("%s: chunk %d lists pages [%d, +%d) of %d\n", what, c, C.first_page, C.num_pages, npg);
      bad++;
      continue;
    }
    const int32_t vs = pqhip::plain_value_size(C.column);
    bool eligible = ncp == 0 && vs > 0 && C.host_status == PQH_OK && C.column.max_def == 0 && C.column.max_rep == 0 &&
                    C.num_pages > 0;
    for (int32_t i = 0; i < C.num_pages; i++) {
      const pqh_page& P = pages[C.first_page + i];
      if (P.image_offset < 0 || P.image_len < 0 || P.image_offset + P.image_len > image_space) {
        printf("%s: page %d image [%lld, +%d) outside %lld bytes\n", what, C.first_page + i, (long long)P.image_offset,
               P.image_len, (long long)image_space);
        bad++;
      }
      spans.emplace_back(P.image_offset, P.image_offset + P.image_len);
      eligible = eligible && (P.page_type == PQH_DATA_PAGE || P.page_type == PQH_DATA_PAGE_V2) &&
                 P.encoding == PQH_ENC_PLAIN && P.num_values >= 0 && P.def_levels_byte_length == 0 &&
                 P.rep_levels_byte_length == 0 && int64_t(P.image_len) == int64_t(P.num_values) * vs;
    }
    // (a chunk whose walk failed after some pages is not packed: its listed pages stay aligned)
    for (int32_t i = 0; i < C.num_pages; i++) {
      const pqh_page& P = pages[C.first_page + i];
      const bool first = i == 0;
      const int64_t want = first ? -1 : pages[C.first_page + i - 1].image_offset + pages[C.first_page + i - 1].image_len;
      if (eligible && !first && P.image_offset != want) {
        printf("%s: chunk %d is packable but page %d starts at %lld, not %lld\n", what, c, i, (long long)P.image_offset,
               (long long)want);
        bad++;
      }
      if ((!eligible || first) && P.image_offset % 64 != 0) {
        printf("%s: chunk %d page %d starts at %lld, not 64-byte aligned\n", what, c, i, (long long)P.image_offset);
        bad++;
      }
    }
    packed += eligible;
  }
  for (int32_t i = 0; i < ncp; i++) {
    if (cps[i].src_offset < 0 || cps[i].src_len < 0 || cps[i].src_offset + cps[i].src_len > payload) {
      printf("%s: codec page %d source [%lld, +%d) outside %lld bytes\n", what, i, (long long)cps[i].src_offset,
             cps[i].src_len, (long long)payload);
      bad++;
    }
    src_spans.emplace_back(cps[i].src_offset, cps[i].src_offset + cps[i].src_len);
  }
  for (auto* v : {&spans, &src_spans}) {
    std::sort(v->begin(), v->end());
    for (size_t i = 1; i < v->size(); i++)
      if ((*v)[i].first < (*v)[i - 1].second) {
        printf("%s: [%lld, %lld) overlaps [%lld, %lld)\n", what, (long long)(*v)[i].first, (long long)(*v)[i].second,
               (long long)(*v)[i - 1].first, (long long)(*v)[i - 1].second);
        bad++;
      }
  }
  // every payload byte, pad included; outside the images (host codecs) / sources (device codecs) all zero
  const uint8_t* p = pqh_host_batch_payload(hb);
  const auto& used = ncp ? src_spans : spans;
  uint64_t sum = 0;
  int64_t stray = 0;
  size_t k = 0;
  for (int64_t i = 0; i < payload + PQH_PAYLOAD_PAD; i++) {
    sum += p[i];
    while (k < used.size() && used[k].second <= i) k++;
    if (!(k < used.size() && used[k].first <= i) && p[i] != 0) stray++;
  }
  if (stray) {
    printf("%s: %lld non-zero bytes outside every page\n", what, (long long)stray);
    bad++;
  }
  printf("%s: %d chunks (%d packed), %d pages, %d codec pages, %lld payload bytes, byte sum %llu: %s\n", what, nch,
         packed, npg, ncp, (long long)payload, (unsigned long long)sum, bad ? "FAILED" : "ok");
  pqh_host_batch_free(hb);
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.parquet\n", argv[0]);
    return 2;
  }
  pqh_file* f = nullptr;
  if (pqh_file_open(argv[1], &f) != PQH_OK) {
    fprintf(stderr, "cannot open %s: %s\n", argv[1], pqh_file_error(f));
    pqh_file_close(f);
    return 2;
  }
  int bad = check_load(f, 0, "host codecs");
  setenv("PQH_DEVICE_CODEC_MAX_RATIO", "0", 1);  // every page of a SNAPPY chunk travels compressed
  bad += check_load(f, PQH_LOAD_DEVICE_SNAPPY, "device snappy");
  pqh_file_close(f);
  return bad ? 1 : 0;
}
