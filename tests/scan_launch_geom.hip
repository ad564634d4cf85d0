// Prints the launch geometry of scan_kernel (ts_scan_dev.h: ts_scan_admits / ts_scan_geom) for every storage format.
// Built and read by tests/test_scan_launch_host.py.  Host arithmetic only: no HIP call, no device needed.
#include <stdio.h>

#include "ts_scan_dev.h"

static void combo(const char* fmt, int d, int kib, bool masked) {
  const size_t stage = sizeof(StageLds);
  const int64_t nworks[] = {1, 8, 9, 100000};
  for (int qh = 1; qh <= 2; ++qh)
    for (int mode = SCAN_DENSE; mode <= SCAN_FILTER; ++mode) {
      if (!ts_scan_admits(kib, qh, stage)) {
        printf("%s d=%d kib=%d qh=%d mode=%d masked=%d refused\n", fmt, d, kib, qh, mode, (int)masked);
        continue;
      }
      for (int64_t nwork : nworks) {
        const TsScanGeom g = ts_scan_geom(kib, qh, mode, masked, stage, nwork, 256);
        printf("%s d=%d kib=%d qh=%d mode=%d masked=%d nwork=%lld -> mode=%d lds=%zu grid=%d\n", fmt, d, kib, qh, mode,
               (int)masked, (long long)nwork, g.mode, g.lds, g.grid);
      }
    }
}

int main() {
  printf("stage %zu\n", sizeof(StageLds));
  const int dims[] = {16, 128, 768, 1024, 1040, 2048, 4096};
  for (int masked = 0; masked <= 1; ++masked) {
    for (int d : dims) {
      combo("f16", d, ts_make_layout(d, TS_F16).kg, masked);
      combo("bf16", d, ts_make_layout(d, TS_BF16).kg, masked);
      if (!masked) combo("f32", d, ts_make_layout(d, TS_F32).kg, false);   // (fp32 storage has no masked scan)
      combo("fp8", d, 2 * ts_make_layout(d, TS_FP8_E4M3).kg, masked);
      if (d <= 2048) combo("fp4", d, ts_make_layout(d, TS_MXFP4_E2M1).qkg, masked);
    }
    const int prefix_kg[] = {8, 16, 48};
    for (int kg : prefix_kg) combo("prefix", 16 * kg, kg, masked);
  }
  return 0;
}
