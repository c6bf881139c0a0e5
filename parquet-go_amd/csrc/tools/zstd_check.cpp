// zstd_check.cpp — stand-alone driver for the host ZSTD decoder (host/codec.cpp zstd_decompress /
// decompress_into over kernels/zstd_core.h).  Reads a corpus written by tests/zstd_blocks.py
// (dump_corpus), decodes every stream into an exactly sized heap buffer, and compares status and
// bytes with what the corpus expects.  Meant to be built with -fsanitize=address,undefined and run
// by hand:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       csrc/tools/zstd_check.cpp csrc/host/codec.cpp -lz -o zstd_check && ./zstd_check corpus.bin
// With --time N it decodes the valid streams N times and prints the single-core rate.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../host/codec.h"

struct Case {
  std::string name;
  std::vector<uint8_t> src, want;
  uint64_t size;
  bool valid;
};

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s corpus.bin [--time N]\n", argv[0]);
    return 2;
  }
  int reps = 0;
  if (argc >= 4 && !strcmp(argv[2], "--time")) reps = atoi(argv[3]);
  FILE* f = fopen(argv[1], "rb");
  char magic[4];
  uint32_t count;
  if (!f || !read_exact(f, magic, 4) || memcmp(magic, "ZSTC", 4) || !read_exact(f, &count, 4)) {
    fprintf(stderr, "cannot read corpus %s\n", argv[1]);
    return 2;
  }
  std::vector<Case> cases(count);
  for (Case& c : cases) {
    uint32_t n, valid;
    bool ok = read_exact(f, &n, 4);
    c.name.resize(ok ? n : 0);
    ok = ok && read_exact(f, &c.name[0], n) && read_exact(f, &n, 4);
    c.src.resize(ok ? n : 0);
    ok = ok && read_exact(f, c.src.data(), n) && read_exact(f, &c.size, 8) && read_exact(f, &valid, 4);
    c.valid = ok && valid;
    if (c.valid) {
      c.want.resize(c.size);
      ok = read_exact(f, c.want.data(), c.size);
    }
    if (!ok) {
      fprintf(stderr, "corpus truncated\n");
      return 2;
    }
  }
  fclose(f);
  int bad = 0, accepted = 0;
  for (const Case& c : cases) {
    // exactly sized heap copies: any read or write outside them is an ASan report
    std::unique_ptr<uint8_t[]> src(new uint8_t[c.src.size()]), dst(new uint8_t[c.size]);
    if (!c.src.empty()) memcpy(src.get(), c.src.data(), c.src.size());
    const bool ok = pqhip::decompress_into(6, src.get(), c.src.size(), dst.get(), size_t(c.size));
    std::vector<uint8_t> grown;
    const bool ok2 = pqhip::decompress_block(6, src.get(), c.src.size(), size_t(c.size / 3), grown);
    if (ok != c.valid || (ok && c.size && memcmp(dst.get(), c.want.data(), c.size))) {
      printf("MISMATCH %s: decoder %s, corpus %s\n", c.name.c_str(), ok ? "accepts" : "rejects",
             c.valid ? "accepts" : "rejects");
      bad++;
    }
    // the growing variant agrees whenever the page size is the stream's own size
    if (ok && (!ok2 || grown.size() != c.size || (c.size && memcmp(grown.data(), c.want.data(), c.size)))) {
      printf("MISMATCH %s: decompress_block differs from decompress_into\n", c.name.c_str());
      bad++;
    }
    accepted += ok;
  }
  printf("%u cases, %d accepted, %d mismatches\n", count, accepted, bad);
  if (reps > 0) {
    uint64_t bytes = 0;
    std::vector<uint8_t> dst;
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; r++)
      for (const Case& c : cases)
        if (c.valid) {
          dst.resize(c.size);
          pqhip::decompress_into(6, c.src.data(), c.src.size(), dst.data(), size_t(c.size));
          bytes += c.size;
        }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%.3f GB/s of output, one core (%llu bytes in %.3f s)\n", double(bytes) / s / 1e9,
           (unsigned long long)bytes, s);
  }
  return bad ? 1 : 0;
}
