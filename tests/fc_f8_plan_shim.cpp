// Host build of mnc_amd/csrc/fc_f8_plan.h for tests/test_f8_host.py (g++ -O2 -shared -fPIC).
#include <cstring>

#include "../mnc_amd/csrc/fc_f8_plan.h"

extern "C" int f8_plan_tune_count() { return mnc::T_COUNT; }
extern "C" int f8_plan_tune_unset() { return mnc::kTuneUnset; }
extern "C" int f8_plan_tune_key(const char* name) {
  static const char* const names[] = {
#define MNC_TUNE_NAME(n) #n,
      MNC_TUNE_KEYS(MNC_TUNE_NAME)
#undef MNC_TUNE_NAME
  };
  for (int i = 0; i < mnc::T_COUNT; ++i)
    if (!strcmp(names[i], name)) return i;
  return -1;
}

// out = {mt, tn, tm, splits, kper, part_bytes, q_bytes, exp_bytes, in_range, packed_bytes, exp_count, decode}
extern "C" void f8_plan_run(const int* tune, int M, int N, int K, int mstride, int quantise_here, long long* out) {
  const mnc::F8Plan p = mnc::fc_f8_plan(M, N, K, mstride, quantise_here != 0, tune);
  const long long v[12] = {p.mt, p.tn, p.tm, p.splits, p.kper, (long long)p.part_bytes, (long long)p.q_bytes, (long long)p.exp_bytes,
                           p.in_range, (long long)mnc::fc_f8_packed_bytes(N, K), (long long)mnc::fc_f8_exp_count(N), p.decode};
  memcpy(out, v, sizeof v);
}
