// Instance-id and class-id label maps of the voted instances for gfx950 -- utils/vis_seg.py:_convert_pred_to_image (reference:
// lib/utils/vis_seg.py:101-130), the VOC colour lookup (:134-147) and PIL's Image.blend over the photograph (tools/demo.py).
// The reference paints the instances one after the other; here every pixel decides for itself.  Per instance i (list order),
// box = np.round(box).astype(int) clipped to the image, bw / bh its size:
//   hit_i(y, x)      the pixel is in the box and the S x S mask resized to (bh, bw) with cv2's INTER_LINEAR rule (cv_resize.h) is
//                    >= float32(binarize_thresh) there
//   outline_i(y, x)  the four numpy slices cls_img[y1:y2+1, x1-1:x1+1], [y1:y2+1, x2-1:x2+1], [y1-1:y1+1, x1:x2+1], [y2-1:y2+1,
//                    x1:x2+1] = 150; a slice that starts at -1 is EMPTY (x1 == 0 draws no left side at all, and so on)
// The outline of an instance is written after its mask and later instances overwrite earlier ones, so walking the list from the
// LAST instance to the first:  cls = 150 if outline_i else class_i if hit_i, for the first i where either holds (else 0);
// inst = i + 1 for the first i with hit_i (else 0).  tests/test_render_host.py holds this rule against the sequential function.
//
//   render_select_kernel  one workgroup: the records with score >= vis_thresh, in record order (ballot prefix count), as one
//                         descriptor each (rounded clipped box, inverse scale factors, class, record row, id).  No host read-back.
//   render_paint_kernel   one workgroup per 64 x 4 pixel tile (one wave per row segment).  It culls the descriptors to those whose
//                         box, grown by the outline's one pixel to the left and top, meets the tile -- into LDS, in order -- then
//                         every lane walks that list backwards for its pixel and leaves when both images are decided.  The
//                         epilogue writes the labels (one int32 per lane, coalesced along x), their VOC colours computed from the
//                         label's bits, and the blend over the uint8 BGR photograph.
// Latency / store bound: 2.4 MB per label map and 1.8 MB per RGB image at 600 x 1000, ~20 VALU operations per tested instance.
//
// Compiled with -ffp-contract=off: the resize is evaluated in the reference's operation order, and the blend is Pillow's
// (UINT8)((int)a + alpha * ((int)b - (int)a)) in float32 with truncation (tests/test_render_host.py pins it against Pillow over
// all 65 536 pairs) -- a fused multiply-add would round once instead of twice.
#include <cmath>
#include <vector>

#include "cv_resize.h"
#include "mnc_internal.h"

namespace mnc {

constexpr int kRenderTileW = 64, kRenderTileH = 4, kRenderThreads = kRenderTileW * kRenderTileH;
constexpr int kRenderMaxMask = 32;             // S <= 32 (cfg.MASK_SIZE is 21)
constexpr double kRenderMaxCoord = 1 << 24;    // |rounded coordinate| limit
constexpr int kRenderMaxSide = 32768;          // H, W limit: the tile grid fits the launch limits, H * W * 4 fits a size_t easily
constexpr int kRenderLdsDescs = 256;           // culled descriptors staged in LDS per tile (12 KB); more -> walk the global list
constexpr int kRenderOutline = 150;

struct alignas(16) RenderDesc {
  int x1, y1, x2, y2;   // rounded, clipped; x2 < x1 or y2 < y1: covers nothing, draws nothing
  int cls, row, id;     // class id, row of the mask array, 0-based position in the painted list
  int pad;
  double ifx, ify;      // cv_inv(bw, S), cv_inv(bh, S)
};
static_assert(sizeof(RenderDesc) == 48, "three 16-byte pieces");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ bool desc_empty(const RenderDesc& d) { return d.x2 < d.x1 || d.y2 < d.y1; }

// block 256.  d_records [record_cap][6 + S*S], rows [0, min(d_counts[0], record_cap)); descs [record_cap]; *d_kept = rows kept.
__global__ __launch_bounds__(256) void render_select_kernel(const float* __restrict__ records, const int* __restrict__ counts,
                                                            int record_cap, int S, double vis_thresh, int H, int W,
                                                            RenderDesc* __restrict__ descs, int* __restrict__ d_kept) {
  __shared__ int wave_cnt[4];
  const int D = 6 + S * S;
  const int n = min(max(counts[0], 0), record_cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int r0 = 0; r0 < n; r0 += 256) {
    const int r = r0 + threadIdx.x;
    const float* rec = records + (long)(r < n ? r : 0) * D;
    // det[:, -1] >= vis_thresh on the reference's float64 boxes: the float32 score widened
    const bool keep = r < n && (double)rec[4] >= vis_thresh;
    const unsigned long long b = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int off = base, total = 0;
    for (int k = 0; k < 4; ++k) {
      if (k < wave) off += wave_cnt[k];
      total += wave_cnt[k];
    }
    if (keep) {
      const int id = off + __popcll(b & ((1ull << lane) - 1ull));
      RenderDesc d;
      // np.round(box).astype(int), half to even (the record holds integral float32 coordinates), then the clip
      d.x1 = clampi((int)rintf(rec[0]), 0, W - 1); d.y1 = clampi((int)rintf(rec[1]), 0, H - 1);
      d.x2 = clampi((int)rintf(rec[2]), 0, W - 1); d.y2 = clampi((int)rintf(rec[3]), 0, H - 1);
      // the record's class id is cls_ind of vis_seg._prepare_dict (over all classes) and cls_ind + 1 of demo.get_vis_dict (over
      // the foreground list): the same number
      d.cls = (int)rec[5];
      d.row = r; d.id = id; d.pad = 0;
      d.ifx = d.x2 >= d.x1 ? cv_inv(d.x2 - d.x1 + 1, S) : 0.0;
      d.ify = d.y2 >= d.y1 ? cv_inv(d.y2 - d.y1 + 1, S) : 0.0;
      descs[id] = d;
    }
    base += total;
    __syncthreads();                      // wave_cnt[] is written again
  }
  if (threadIdx.x == 0) *d_kept = base;
}

// r, g, b of _get_voc_color_map()[label]: bit (7 - j) of (r, g, b) from bits (3j, 3j + 1, 3j + 2) of the label.  Labels are below
// 256 there, so j = 0..2 carry everything (bits 8.. are zero).
__device__ __forceinline__ void voc_colour(int label, int& r, int& g, int& b) {
  r = g = b = 0;
  int cid = label & 255;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    r |= ((cid >> 0) & 1) << (7 - j);
    g |= ((cid >> 1) & 1) << (7 - j);
    b |= ((cid >> 2) & 1) << (7 - j);
    cid >>= 3;
  }
}

// Pillow's ImagingBlend for 8-bit channels, 0 <= alpha <= 1 (no clipping branch): float32 arithmetic, truncation
__device__ __forceinline__ unsigned char pil_blend(int a, int b, float alpha) {
  const float t = (float)a + alpha * (float)(b - a);
  return (unsigned char)(int)t;
}

// The rule at one pixel over descriptors list[0 .. n) (LDS or global), walked backwards.
__device__ __forceinline__ void paint_px(const RenderDesc* list, int n, const float* __restrict__ masks, long mask_stride, int S,
                                         float mthr, int y, int x, int& inst, int& cls) {
  bool di = false, dc = false;
  inst = 0; cls = 0;
  for (int j = n - 1; j >= 0; --j) {
    const RenderDesc& d = list[j];
    if (desc_empty(d)) continue;
    const bool in_x = x >= d.x1 && x <= d.x2, in_y = y >= d.y1 && y <= d.y2;
    bool outline = false;
    if (!dc) {
      const bool side = in_y && ((d.x1 > 0 && x >= d.x1 - 1 && x <= d.x1) || (d.x2 > 0 && x >= d.x2 - 1 && x <= d.x2));
      const bool cap = in_x && ((d.y1 > 0 && y >= d.y1 - 1 && y <= d.y1) || (d.y2 > 0 && y >= d.y2 - 1 && y <= d.y2));
      outline = side || cap;
    }
    bool hit = false;
    if (in_x && in_y && (!di || (!dc && !outline)))
      hit = cv_px(masks + (long)d.row * mask_stride, S, y - d.y1, x - d.x1, d.ifx, d.ify) >= mthr;
    if (!dc) {
      if (outline) { cls = kRenderOutline; dc = true; }
      else if (hit) { cls = d.cls; dc = true; }
    }
    if (!di && hit) { inst = d.id + 1; di = true; }
    if (di && dc) break;
  }
}

// grid (ceil(W / 64), ceil(H / 4)), block 256.  descs [n]: n = *d_n when d_n is given, else n_fixed.  Mask of descriptor d:
// masks + d.row * mask_stride, S * S float32.  Every output may be null; bgr is the uint8 [H][W][3] photograph (null: black).
__global__ __launch_bounds__(kRenderThreads) void render_paint_kernel(
    const RenderDesc* __restrict__ descs, const int* __restrict__ d_n, int n_fixed, const float* __restrict__ masks,
    long mask_stride, int S, float mthr, int H, int W, const unsigned char* __restrict__ bgr, float alpha,
    int* __restrict__ inst_img, int* __restrict__ cls_img, unsigned char* __restrict__ inst_rgb,
    unsigned char* __restrict__ cls_rgb, unsigned char* __restrict__ overlay_rgb) {
  __shared__ RenderDesc lds[kRenderLdsDescs];
  __shared__ int wave_cnt[4];
  const int n = d_n ? *d_n : n_fixed;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx0 = blockIdx.x * kRenderTileW, ty0 = blockIdx.y * kRenderTileH;
  const int tx1 = tx0 + kRenderTileW - 1, ty1 = ty0 + kRenderTileH - 1;
  // cull, in list order
  int culled = 0;
  for (int c0 = 0; c0 < n; c0 += kRenderThreads) {
    const int i = c0 + threadIdx.x;
    bool meets = false;
    if (i < n) {
      const int4 b = *reinterpret_cast<const int4*>(&descs[i]);      // x1, y1, x2, y2
      meets = b.z >= b.x && b.w >= b.y && b.x - 1 <= tx1 && b.z >= tx0 && b.y - 1 <= ty1 && b.w >= ty0;
    }
    const unsigned long long b = __ballot(meets);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int off = culled, total = 0;
    for (int k = 0; k < 4; ++k) {
      if (k < wave) off += wave_cnt[k];
      total += wave_cnt[k];
    }
    if (meets) {
      const int slot = off + __popcll(b & ((1ull << lane) - 1ull));
      if (slot < kRenderLdsDescs) {
        const int4* src = reinterpret_cast<const int4*>(&descs[i]);
        int4* dst = reinterpret_cast<int4*>(&lds[slot]);
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
      }
    }
    culled += total;
    __syncthreads();
  }
  const int x = tx0 + lane, y = ty0 + wave;
  if (x >= W || y >= H) return;
  int inst, cls;
  if (culled <= kRenderLdsDescs) paint_px(lds, culled, masks, mask_stride, S, mthr, y, x, inst, cls);
  else paint_px(descs, n, masks, mask_stride, S, mthr, y, x, inst, cls);
  const long p = (long)y * W + x;
  if (inst_img) inst_img[p] = inst;
  if (cls_img) cls_img[p] = cls;
  if (inst_rgb) {
    int r, g, b;
    voc_colour(inst, r, g, b);
    inst_rgb[3 * p] = (unsigned char)r; inst_rgb[3 * p + 1] = (unsigned char)g; inst_rgb[3 * p + 2] = (unsigned char)b;
  }
  if (cls_rgb || overlay_rgb) {
    int r, g, b;
    voc_colour(cls, r, g, b);
    if (cls_rgb) { cls_rgb[3 * p] = (unsigned char)r; cls_rgb[3 * p + 1] = (unsigned char)g; cls_rgb[3 * p + 2] = (unsigned char)b; }
    if (overlay_rgb) {
      // Image.blend(photo as RGB, cls_rgb, alpha): the photograph is BGR
      const int pb = bgr ? bgr[3 * p] : 0, pg = bgr ? bgr[3 * p + 1] : 0, pr = bgr ? bgr[3 * p + 2] : 0;
      overlay_rgb[3 * p] = pil_blend(pr, r, alpha);
      overlay_rgb[3 * p + 1] = pil_blend(pg, g, alpha);
      overlay_rgb[3 * p + 2] = pil_blend(pb, b, alpha);
    }
  }
}

namespace {

void paint_launch(hipStream_t s, const RenderDesc* d_descs, const int* d_n, int n_fixed, const float* d_masks, long mask_stride,
                  int S, double binarize_thresh, int H, int W, const unsigned char* d_bgr, float alpha, int* d_inst, int* d_cls,
                  unsigned char* d_inst_rgb, unsigned char* d_cls_rgb, unsigned char* d_overlay_rgb) {
  const dim3 grid((W + kRenderTileW - 1) / kRenderTileW, (H + kRenderTileH - 1) / kRenderTileH);
  // a numpy float32 mask is compared with the Python float threshold in float32
  hipLaunchKernelGGL(render_paint_kernel, grid, dim3(kRenderThreads), 0, s, d_descs, d_n, n_fixed, d_masks, mask_stride, S,
                     (float)binarize_thresh, H, W, d_bgr, alpha, d_inst, d_cls, d_inst_rgb, d_cls_rgb, d_overlay_rgb);
}

// per-context descriptor scratch (mnc_ctx::render_ws): [kept count: 256 B | record_cap descriptors].  No captured graph holds its
// address (rendering is never part of one), so growing it does not touch mnc_ctx::arena_gen.
int ctx_render_ws(mnc_ctx* ctx, int record_cap, int** d_kept, RenderDesc** d_descs) {
  auto layout = [&](WsLayout l) {
    *d_kept = l.take<int>(1);
    *d_descs = l.take<RenderDesc>(record_cap > 0 ? record_cap : 1);
    return l.bytes();
  };
  const int rc = arena_ensure(&ctx->render_ws, layout(WsLayout()), 0, "render scratch", ctx->stream, ctx);
  if (rc) return rc;
  layout(WsLayout(ctx->render_ws.p));
  return MNC_OK;
}

}  // namespace

}  // namespace mnc

using namespace mnc;

// see include/mnc_hip.h
int mnc_render_instances(const double* boxes, const float* masks, const int* classes, int n, int mask_size, double binarize_thresh,
                         int image_height, int image_width, int* inst_img, int* cls_img, int device_id) {
  const int H = image_height, W = image_width, S = mask_size;
  MNC_REQUIRE(n >= 0, "mnc_render_instances: n=%d must be >= 0", n);
  MNC_REQUIRE(S >= 1 && S <= kRenderMaxMask, "mnc_render_instances: mask_size %d not in [1, %d]", S, kRenderMaxMask);
  MNC_REQUIRE(H >= 2 && W >= 2 && H <= kRenderMaxSide && W <= kRenderMaxSide,
              "mnc_render_instances: image %d x %d not in [2, %d] (a slice starting at -1 must be empty, not wrapped)", H, W,
              kRenderMaxSide);
  MNC_REQUIRE(n == 0 || (boxes && masks && classes), "mnc_render_instances: null pointer");
  std::vector<RenderDesc> descs((size_t)n);
  for (int i = 0; i < n; ++i) {
    const double* b = boxes + 4 * (size_t)i;
    int q[4];
    for (int k = 0; k < 4; ++k) {
      const double r = std::rint(b[k]);                // np.round: half to even
      MNC_REQUIRE(std::fabs(r) < kRenderMaxCoord, "mnc_render_instances: box %d coordinate %g out of range", i, b[k]);
      const int hi = (k & 1) ? H - 1 : W - 1;
      const int v = (int)r;
      q[k] = v < 0 ? 0 : v > hi ? hi : v;
    }
    MNC_REQUIRE(q[0] <= q[2] && q[1] <= q[3],
                "mnc_render_instances: box %d (%g, %g, %g, %g) is empty once rounded and clipped (cv2.resize would raise)", i, b[0],
                b[1], b[2], b[3]);
    RenderDesc& d = descs[i];
    d.x1 = q[0]; d.y1 = q[1]; d.x2 = q[2]; d.y2 = q[3];
    d.cls = classes[i]; d.row = i; d.id = i; d.pad = 0;
    d.ifx = 1.0 / ((double)(q[2] - q[0] + 1) / (double)S);
    d.ify = 1.0 / ((double)(q[3] - q[1] + 1) / (double)S);
  }
  if (!inst_img && !cls_img) { clear_error(); return MNC_OK; }
  const size_t px = (size_t)H * W;
  RenderDesc* d_descs; float* d_masks; int *d_inst, *d_cls;
  auto layout = [&](WsLayout l) {
    d_descs = l.take<RenderDesc>(n);
    d_masks = l.take<float>((size_t)n * S * S);
    d_inst = l.take<int>(px);
    d_cls = l.take<int>(px);
    return l.bytes();
  };
  HostScope hs;
  int rc = hs.open(device_id, layout(WsLayout()));
  if (rc) return rc;
  layout(WsLayout(hs.buf));
  MNC_HIP_TRY(hs.up(d_descs, descs.data(), (size_t)n * sizeof(RenderDesc)));
  MNC_HIP_TRY(hs.up(d_masks, masks, (size_t)n * S * S * 4));
  paint_launch(hs.stream, d_descs, nullptr, n, d_masks, (long)S * S, S, binarize_thresh, H, W, nullptr, 0.0f,
               inst_img ? d_inst : nullptr, cls_img ? d_cls : nullptr, nullptr, nullptr, nullptr);
  MNC_HIP_TRY(hipGetLastError());
  if (inst_img) MNC_HIP_TRY(hs.down(inst_img, d_inst, px * 4));
  if (cls_img) MNC_HIP_TRY(hs.down(cls_img, d_cls, px * 4));
  MNC_HIP_TRY(hs.sync());
  clear_error();
  return MNC_OK;
}

// see include/mnc_hip.h
int mnc_render_records(mnc_ctx* ctx, const float* d_records, const int* d_counts, int record_cap, int num_classes, int mask_size,
                       double vis_thresh, double binarize_thresh, int H, int W, const unsigned char* d_bgr_hwc, float alpha,
                       int* d_inst, int* d_cls, unsigned char* d_inst_rgb, unsigned char* d_cls_rgb, unsigned char* d_overlay_rgb,
                       int* d_kept) {
  MNC_REQUIRE(ctx && d_records && d_counts, "mnc_render_records: null pointer");
  MNC_REQUIRE(record_cap >= 0 && num_classes >= 1 && num_classes <= 256, "mnc_render_records: record_cap=%d, num_classes=%d",
              record_cap, num_classes);
  MNC_REQUIRE(mask_size >= 1 && mask_size <= kRenderMaxMask, "mnc_render_records: mask_size %d not in [1, %d]", mask_size,
              kRenderMaxMask);
  MNC_REQUIRE(H >= 2 && W >= 2 && H <= kRenderMaxSide && W <= kRenderMaxSide, "mnc_render_records: image %d x %d not in [2, %d]", H,
              W, kRenderMaxSide);
  MNC_REQUIRE(alpha >= 0.0f && alpha <= 1.0f, "mnc_render_records: alpha %g not in [0, 1]", (double)alpha);
  int* ws_kept = nullptr;
  RenderDesc* descs = nullptr;
  int rc = ctx_render_ws(ctx, record_cap, &ws_kept, &descs);
  if (rc) return rc;
  const int S = mask_size;
  LaunchScope ls(ctx, "render");
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(render_select_kernel, dim3(1), dim3(256), 0, s, d_records, d_counts, record_cap, S, vis_thresh, H, W, descs,
                     ws_kept);
  if (d_inst || d_cls || d_inst_rgb || d_cls_rgb || d_overlay_rgb)
    paint_launch(s, descs, ws_kept, 0, d_records + 6, 6 + (long)S * S, S, binarize_thresh, H, W, d_bgr_hwc, alpha, d_inst, d_cls,
                 d_inst_rgb, d_cls_rgb, d_overlay_rgb);
  rc = ls.finish("render");
  if (rc) return rc;
  if (d_kept) MNC_HIP_TRY(hipMemcpyAsync(d_kept, ws_kept, sizeof(int), hipMemcpyDeviceToDevice, s));
  clear_error();
  return MNC_OK;
}
