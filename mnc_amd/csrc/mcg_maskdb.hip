// The MCG proposal maskdb of the CFM task for gfx950 -- the validation branch of the reference's tools/prepare_mcg_maskdb.py:55-97.
// One image: a superpixel label map [H][W] and n proposals, each a list of superpixel ids (CSR: label_ptr / label_ids).  With P_i
// the pixels whose id is in list i (np.in1d; duplicates and ids that occur nowhere change nothing):
//   box_i   [min col, min row, max col, max row] of P_i, as float64
//   mask_i  cv2.resize(P_i[y1:y2+1, x1:x2+1], (S, S), INTER_NEAREST): mask[dy][dx] = P_i[y1 + sy(dy)][x1 + sx(dx)] with
//           sx(dx) = min(floor(dx * ifx), w - 1), ifx = 1.0 / ((double)S / w) -- OpenCV's resizeNN forms the inverse scale in two
//           steps and then takes cvFloor; this differs from dx * w / S in integers and from dx * (w / (double)S).  The rule rests on
//           OpenCV's published source (imgproc/src/resize.cpp), as the bilinear restatement in cv_resize.h does.
// No per-proposal image is ever built: the extent of a union is the extent of its superpixels' extents, and the S x S samples are
// S * S lookups into the label map.
//
// mcg_extent_kernel: one pass over the label map fills table[id] = (min x, min y, -max x, -max y) with integer atomicMin.  Only
//   pixels on the border of their superpixel can hold an extreme (the pixel with the smallest x of a superpixel has another id, or
//   the image edge, on its left, and so on), so only those issue an atomic: ~4 * sqrt(area) per superpixel instead of 4 * area.
//   Integer minima are order-free: the table is deterministic.  The maxima are kept negated so that one byte fill (0x7f) makes
//   every field "empty".
// mcg_mask_kernel: one workgroup (256 lanes) per proposal.  The list's membership bitset goes to LDS (one bit per id of the map),
//   the members' table entries are reduced with wave shuffles (an id that occurs nowhere has an empty entry, which is the identity
//   of min), then the S * S samples are one label-map read and one bit test each.  An empty union puts the proposal's index into
//   the call's error word with atomicMin; the host reads it back with the results.
// Bound: latency -- one fill, two launches, three copies each way; the kernels move ~1 MB.
//
// Not in _build.py's NO_CONTRACT list: the only floating-point expressions are a float64 division, a reciprocal and the product
// dx * ifx, which is followed by floor -- there is no addition a multiply could be contracted with.
#include <algorithm>

#include "cv_resize.h"
#include "mnc_internal.h"

namespace mnc {

constexpr int kMcgThreads = 256;
constexpr int kMcgMaxMask = 32;          // S <= 32 (the maskdb's S is 21)
constexpr int kMcgMaxSide = 32768;       // H, W
constexpr int kMcgMaxId = 65535;         // MCG's label maps are uint16
constexpr int kMcgEmpty = 0x7f7f7f7f;    // a table field / the error word after the 0x7f byte fill

// table [max_id + 1][4] filled with kMcgEmpty; every id of sp is in [0, max_id] (checked by the host)
__global__ __launch_bounds__(kMcgThreads) void mcg_extent_kernel(const int* __restrict__ sp, int H, int W, int* __restrict__ table) {
  const int total = H * W, stride = gridDim.x * kMcgThreads;
  for (int i = blockIdx.x * kMcgThreads + threadIdx.x; i < total; i += stride) {
    const int y = i / W, x = i - y * W;
    const int id = sp[i];
    int* t = table + 4 * id;
    if (x == 0 || sp[i - 1] != id) atomicMin(t, x);
    if (y == 0 || sp[i - W] != id) atomicMin(t + 1, y);
    if (x == W - 1 || sp[i + 1] != id) atomicMin(t + 2, -x);
    if (y == H - 1 || sp[i + W] != id) atomicMin(t + 3, -y);
  }
}

__global__ __launch_bounds__(kMcgThreads) void mcg_mask_kernel(const int* __restrict__ sp, int W, const int* __restrict__ label_ptr,
                                                               const int* __restrict__ label_ids, const int4* __restrict__ table,
                                                               int max_id, int S, double* __restrict__ boxes,
                                                               unsigned char* __restrict__ masks, int* __restrict__ err) {
  __shared__ unsigned bits[(kMcgMaxId + 1) / 32];
  __shared__ int red[kMcgThreads / 64][4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int words = (max_id >> 5) + 1;
  for (int i = tid; i < words; i += kMcgThreads) bits[i] = 0u;
  __syncthreads();
  int x1 = kMcgEmpty, y1 = kMcgEmpty, nx2 = kMcgEmpty, ny2 = kMcgEmpty;
  const int k1 = label_ptr[p + 1];
  for (int k = label_ptr[p] + tid; k < k1; k += kMcgThreads) {
    const int id = label_ids[k];
    if (id > max_id) continue;                               // above every id of the map: occurs nowhere
    atomicOr(&bits[id >> 5], 1u << (id & 31));
    const int4 e = table[id];
    x1 = min(x1, e.x); y1 = min(y1, e.y); nx2 = min(nx2, e.z); ny2 = min(ny2, e.w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x1 = min(x1, __shfl_xor(x1, o)); y1 = min(y1, __shfl_xor(y1, o));
    nx2 = min(nx2, __shfl_xor(nx2, o)); ny2 = min(ny2, __shfl_xor(ny2, o));
  }
  if ((tid & 63) == 0) { int* r = red[tid >> 6]; r[0] = x1; r[1] = y1; r[2] = nx2; r[3] = ny2; }
  __syncthreads();                                           // also: the bitset is complete
#pragma unroll
  for (int k = 0; k < kMcgThreads / 64; ++k) {
    x1 = min(x1, red[k][0]); y1 = min(y1, red[k][1]); nx2 = min(nx2, red[k][2]); ny2 = min(ny2, red[k][3]);
  }
  if (x1 == kMcgEmpty) {                                     // uniform over the block: P is empty (np.min would raise)
    if (tid == 0) atomicMin(err, p);
    return;
  }
  const int x2 = -nx2, y2 = -ny2, w = x2 - x1 + 1, h = y2 - y1 + 1;
  if (tid == 0) {
    double* b = boxes + 4 * (size_t)p;
    b[0] = x1; b[1] = y1; b[2] = x2; b[3] = y2;
  }
  const double ifx = cv_inv(S, w), ify = cv_inv(S, h);
  unsigned char* m = masks + (size_t)p * S * S;
  for (int i = tid; i < S * S; i += kMcgThreads) {
    const int dy = i / S, dx = i - dy * S;
    const int sx = min((int)floor(dx * ifx), w - 1), sy = min((int)floor(dy * ify), h - 1);
    const int id = sp[(y1 + sy) * W + x1 + sx];
    m[i] = (bits[id >> 5] >> (id & 31)) & 1u;
  }
}

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_mcg_maskdb(const int* superpixels, int H, int W, const int* label_ptr, const int* label_ids, int n, int mask_size,
                   double* boxes, unsigned char* masks, int device_id) {
  MNC_REQUIRE(n >= 0, "mnc_mcg_maskdb: n=%d must be >= 0", n);
  MNC_REQUIRE(mask_size >= 1 && mask_size <= kMcgMaxMask, "mnc_mcg_maskdb: mask_size %d not in [1, %d]", mask_size, kMcgMaxMask);
  MNC_REQUIRE(H >= 1 && H <= kMcgMaxSide && W >= 1 && W <= kMcgMaxSide, "mnc_mcg_maskdb: H=%d, W=%d not in [1, %d]", H, W,
              kMcgMaxSide);
  if (n == 0) { clear_error(); return MNC_OK; }
  MNC_REQUIRE(superpixels && label_ptr && label_ids && boxes && masks, "mnc_mcg_maskdb: null pointer");
  MNC_REQUIRE(label_ptr[0] == 0, "mnc_mcg_maskdb: label_ptr[0] = %d must be 0", label_ptr[0]);
  for (int i = 0; i < n; ++i)
    MNC_REQUIRE(label_ptr[i] <= label_ptr[i + 1], "mnc_mcg_maskdb: label_ptr decreases at proposal %d (%d -> %d)", i, label_ptr[i],
                label_ptr[i + 1]);
  const size_t px = (size_t)H * W, L = (size_t)label_ptr[n];
  int lo = 0, max_id = 0;
  for (size_t i = 0; i < px; ++i) { lo = std::min(lo, superpixels[i]); max_id = std::max(max_id, superpixels[i]); }
  MNC_REQUIRE(lo >= 0 && max_id <= kMcgMaxId, "mnc_mcg_maskdb: superpixel ids span [%d, %d], outside [0, %d]", lo, max_id, kMcgMaxId);
  int llo = 0, lhi = 0;
  for (size_t i = 0; i < L; ++i) { llo = std::min(llo, label_ids[i]); lhi = std::max(lhi, label_ids[i]); }
  MNC_REQUIRE(llo >= 0 && lhi <= kMcgMaxId, "mnc_mcg_maskdb: label ids span [%d, %d], outside [0, %d]", llo, lhi, kMcgMaxId);

  const int S = mask_size;
  const size_t nP = (size_t)n, table_bytes = ((size_t)max_id + 1) * 16;
  int *d_sp, *d_ptr, *d_ids, *d_table; double* d_boxes; unsigned char* d_masks;
  auto layout = [&](WsLayout l) {
    d_sp = l.take<int>(px);
    d_ptr = l.take<int>(nP + 1);
    d_ids = l.take<int>(L);
    d_table = l.take<int>(table_bytes / 4 + 1);     // the error word follows the table
    d_boxes = l.take<double>(nP * 4);
    d_masks = l.take<unsigned char>(nP * S * S);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, 0);                   // the device's stream (and device check); the buffer is this call's own
  if (rc) return rc;
  CallBuf buf;
  rc = buf.alloc("mnc_mcg_maskdb", layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(buf.p));
  int* d_err = d_table + table_bytes / 4;
  MNC_HIP_TRY(hs.up(d_sp, superpixels, px * 4));
  MNC_HIP_TRY(hs.up(d_ptr, label_ptr, (nP + 1) * 4));
  MNC_HIP_TRY(hs.up(d_ids, label_ids, L * 4));
  MNC_HIP_TRY(hipMemsetAsync(d_table, 0x7f, table_bytes + 4, hs.stream));
  const int grid = std::min(cdiv((long)px, kMcgThreads), 2048);
  hipLaunchKernelGGL(mcg_extent_kernel, dim3(grid), dim3(kMcgThreads), 0, hs.stream, d_sp, H, W, d_table);
  MNC_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mcg_mask_kernel, dim3(n), dim3(kMcgThreads), 0, hs.stream, d_sp, W, d_ptr, d_ids, (const int4*)d_table, max_id, S,
                     d_boxes, d_masks, d_err);
  MNC_HIP_TRY(hipGetLastError());
  int first_empty = kMcgEmpty;
  MNC_HIP_TRY(hs.down(boxes, d_boxes, nP * 32));
  MNC_HIP_TRY(hs.down(masks, d_masks, nP * S * S));
  MNC_HIP_TRY(hs.down(&first_empty, d_err, 4));
  MNC_HIP_TRY(hs.sync());
  MNC_REQUIRE(first_empty == kMcgEmpty,
              "mnc_mcg_maskdb: proposal %d covers no pixel (its list is empty or none of its ids occurs in the label map)", first_empty);
  clear_error();
  return MNC_OK;
}
