// Host cost of dp_gemm_plan alone: a native loop over the list of tools/gemm_plan_table.py (--dump FILE).
//   g++ -O2 -std=c++17 -I include tools/gemm_plan_time.cpp -o /tmp/gemm_plan_time -ldl
//   /tmp/gemm_plan_time <libdp_mi355x.so> <FILE> [passes]      -> seconds per pass, and a checksum of the answers
#include <dlfcn.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dp_mi355x.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
  if (!lib) { std::fprintf(stderr, "%s\n", dlerror()); return 1; }
  auto plan = (int (*)(const dp_gemm_args*, int32_t*, int32_t*))dlsym(lib, "dp_gemm_plan");
  auto flags = (int (*)(int))dlsym(lib, "dp_gemm_debug_flags");
  FILE* fh = std::fopen(argv[2], "rb");
  int64_t hdr[4];
  if (!plan || !flags || !fh || std::fread(hdr, 8, 4, fh) != 4 || hdr[1] != (int64_t)sizeof(dp_gemm_args)) return 1;
  std::vector<dp_gemm_args> args(hdr[0]);
  std::vector<int32_t> blocks(3 * hdr[2]);
  if (std::fread(args.data(), sizeof(dp_gemm_args), args.size(), fh) != args.size() ||
      std::fread(blocks.data(), 4, blocks.size(), fh) != blocks.size()) return 1;
  const int passes = argc > 3 ? std::atoi(argv[3]) : 1;
  for (int pass = 0; pass < passes; ++pass) {
    long long sum = 0, rows = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t b = 0; b < blocks.size(); b += 3) {
      flags(blocks[b]);
      dp_gemm_args a = args[blocks[b + 1]];
      for (int ws = 0; ws < 2; ++ws) {
        a.workspace = ws ? (void*)256 : nullptr;
        a.workspace_bytes = ws ? hdr[3] : 0;
        for (int h = 0; h < blocks[b + 2]; ++h, ++rows) {
          int32_t tile = -1, grid = -1;
          a.tile = h;
          sum += plan(&a, &tile, &grid) + 31LL * tile + grid;
        }
      }
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("pass: %.4f s, %lld rows, %.1f ns per call, checksum %lld\n", s, rows, 1e9 * s / rows, sum);
  }
  flags(0);
  return 0;
}
