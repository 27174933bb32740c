// Stand-alone host check of the resampler's plan code (csrc/resample.hip: plan creation, export, num_output, destroy) for a
// sanitizer build.  Runs on the CPU only: no device is touched (a plan uploads its tables on its first launch, and nothing is
// launched here).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Ipykaldi2_amd/csrc \
//       tools/resample_host_check.cpp pykaldi2_amd/csrc/resample.hip pykaldi2_amd/csrc/abi.hip -o /tmp/resample_host_check \
//     && /tmp/resample_host_check
#include <math.h>
#include <stdio.h>

#include <vector>

#include "pk2hip.h"

static int fail(const char* what) {
  fprintf(stderr, "FAILED: %s (%s)\n", what, pk2_last_error());
  return 1;
}

int main() {
  const int ratios[6][2] = {{14400, 16000}, {17600, 16000}, {16000, 8000}, {8000, 16000}, {48000, 16000}, {15217, 16000}};
  const int first0[6] = {-6, -6, -12, -6, -18, -6};
  for (int r = 0; r < 6; ++r) {
    pk2_resample_plan* plan = nullptr;
    if (pk2_resample_plan_create(ratios[r][0], ratios[r][1], 0.0, 6, &plan) != PK2_OK) return fail("plan_create");
    int32_t iu, ou, max_taps, tile;
    int64_t bytes;
    if (pk2_resample_plan_info(plan, &iu, &ou, &max_taps, &tile, &bytes) != PK2_OK) return fail("plan_info");
    std::vector<int32_t> first(ou), taps(ou);
    std::vector<float> w((size_t)ou * max_taps);
    if (pk2_resample_plan_export(plan, first.data(), taps.data(), w.data()) != PK2_OK) return fail("plan_export");
    double lo = 1e9, hi = -1e9;
    for (int p = 0; p < ou; ++p) {
      double s = 0.0;
      for (int j = 0; j < taps[p]; ++j) s += w[(size_t)p * max_taps + j];
      lo = fmin(lo, s); hi = fmax(hi, s);
    }
    if (first[0] != first0[r] || lo < 0.9999 || hi > 1.0011) return fail("tables");
    for (int64_t n = 1; n <= 200; ++n) {
      const int64_t want = (n * ratios[r][1] + ratios[r][0] - 1) / ratios[r][0];
      if (pk2_resample_num_output(plan, n) != want) return fail("num_output");
    }
    if (pk2_resample_num_output(plan, 1000000000) != (1000000000LL * ratios[r][1] + ratios[r][0] - 1) / ratios[r][0])
      return fail("num_output 1e9");
    printf("%d -> %d: iu %d ou %d max_taps %d tile %d table %lld bytes, phase sums %.5f .. %.5f\n", ratios[r][0], ratios[r][1],
           iu, ou, max_taps, tile, (long long)bytes, lo, hi);
    if (pk2_resample_plan_destroy(plan) != PK2_OK) return fail("plan_destroy");
  }
  pk2_resample_plan* plan = nullptr;
  if (pk2_resample_plan_create(0, 16000, 0.0, 6, &plan) == PK2_OK || plan) return fail("rate 0 accepted");
  if (pk2_resample_plan_create(16000, 8000, 4000.5, 6, &plan) == PK2_OK || plan) return fail("cutoff above Nyquist accepted");
  if (pk2_resample_plan_create(16000, 8000, 0.0, 0, &plan) == PK2_OK || plan) return fail("num_zeros 0 accepted");
  if (pk2_resample_plan_create(16000, 250, 0.0, 6, &plan) == PK2_OK || plan) return fail("ratio beyond the staged span accepted");
  if (pk2_resample_plan_create(16000, 16000, 0.0, 6, &plan) != PK2_OK) return fail("identity plan");
  if (pk2_resample_num_output(plan, 77) != 77 || pk2_resample_plan_destroy(plan) != PK2_OK) return fail("identity plan");
  printf("resample host check ok\n");
  return 0;
}
