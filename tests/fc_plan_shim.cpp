// Host build of mnc_amd/csrc/fc_plan.h for tests/test_fc_plan.py (g++ -O2 -shared -fPIC).
#include <cstring>

#include "../mnc_amd/csrc/fc_plan.h"

extern "C" int fc_plan_tune_count() { return mnc::T_COUNT; }
extern "C" int fc_plan_tune_unset() { return mnc::kTuneUnset; }
extern "C" int fc_plan_tune_key(const char* name) {
  static const char* const names[] = {
#define MNC_TUNE_NAME(n) #n,
      MNC_TUNE_KEYS(MNC_TUNE_NAME)
#undef MNC_TUNE_NAME
  };
  for (int i = 0; i < mnc::T_COUNT; ++i)
    if (!strcmp(names[i], name)) return i;
  return -1;
}

// which: 0 = mnc_fc, 1 = mnc_fc_pair, 2 = fc_lowp, 3 = fc_lowp_pair.  call = {M, N, K, ldc, f16, osm0, osm1, osm_rows, osm_row0, pre0,
// pre1, mstride, defer_reduce, aligned16}; out = {head, two_singles, small, kernel, mt, sk, tn, tm, tm_arg, splits, kper, slab, buf,
// drop, part_bytes, conv_bytes}.
extern "C" void fc_plan_run(int which, int tuning, const int* tune, const long long* call, long long* out) {
  mnc::FcCall c((int)call[0], (int)call[1], (int)call[2], (int)call[3]);
  c.f16 = (int)call[4];
  c.osm[0] = call[5] != 0; c.osm[1] = call[6] != 0; c.osm_rows = (long)call[7]; c.osm_row0 = (long)call[8];
  c.pre[0] = call[9] != 0; c.pre[1] = call[10] != 0; c.mstride = (int)call[11];
  c.defer_reduce = call[12] != 0;
  c.aligned16 = call[13] != 0;
  const mnc::FcPlan p = which == 0 ? mnc::fc_plan(c, tune, tuning != 0) : which == 1 ? mnc::fc_pair_plan(c, tune, tuning != 0)
                        : which == 2 ? mnc::fc_lowp_plan(c, tune) : mnc::fc_lowp_pair_plan(c, tune);
  const long long v[16] = {p.head, p.two_singles, p.small, p.kernel, p.mt, p.sk, p.tn, p.tm, p.tm_arg, p.splits, p.kper, p.slab, p.buf,
                           p.drop, (long long)p.part_bytes, (long long)p.conv_bytes};
  memcpy(out, v, sizeof v);
}
