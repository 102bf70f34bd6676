// Carver of one allocation into typed sub-buffers, each starting on a 256-byte boundary.  No HIP include: tests/test_ws_layout.py
// compiles it for the host.
//
// A layout is written ONCE, as a function of the carver, and run twice: with a null base to size the buffer, then with the
// allocated base to get the pointers -- the size and the pointers cannot disagree.
//   static void my_layout(WsLayout& l, int n, MyWs* w) { w->a = l.take<float>(n); w->b = l.take<int>(4 * n); }
//   WsLayout size;        my_layout(size, n, &w);      ... allocate size.bytes() ...
//   WsLayout at(buffer);  my_layout(at, n, &w);
#pragma once
#include <cstddef>
#include <cstdint>

namespace mnc {

struct WsLayout {
  uintptr_t base;
  size_t off = 0;
  explicit WsLayout(void* b = nullptr) : base((uintptr_t)b) {}
  // `count` elements of T at the running offset (a zero count takes no room: the next member gets the same address)
  template <typename T>
  T* take(size_t count) {
    T* p = (T*)(base + off);
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
  size_t bytes() const { return off; }
};

}  // namespace mnc
