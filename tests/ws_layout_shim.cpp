// Host build of mnc_amd/csrc/ws_layout.h for tests/test_ws_layout.py (g++ -O2 -shared -fPIC).
#include "../mnc_amd/csrc/ws_layout.h"
struct Desc48 { char b[48]; };      // (the size of render.hip's descriptor: not a power of two)
// One layout of n members, member i = counts[i] elements of elem[i] bytes (1, 4, 8 or 48), carved from `base` (may be null).
// addrs[i] = the address take() returned; -> bytes(), or 0 for an element size the shim does not know.
extern "C" size_t ws_layout_run(void* base, const size_t* counts, const int* elem, int n, size_t* addrs) {
  mnc::WsLayout l(base);
  for (int i = 0; i < n; ++i) {
    void* p;
    switch (elem[i]) {
      case 1: p = l.take<unsigned char>(counts[i]); break;
      case 4: p = l.take<int>(counts[i]); break;
      case 8: p = l.take<double>(counts[i]); break;
      case 48: p = l.take<Desc48>(counts[i]); break;
      default: return 0;
    }
    addrs[i] = (size_t)p;
  }
  return l.bytes();
}
