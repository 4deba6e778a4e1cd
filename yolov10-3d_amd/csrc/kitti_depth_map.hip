// Foreground depth maps of a KITTI batch (`load_depth_maps`, data/datasets/kitti.py:143-145, 170-201, 286-287, 384-385, 409-417):
// the instance segmentation mask of every frame (and of its mixup partner) is mirrored with the image, warped with the image's crop
// matrix by Pillow's NEAREST affine transform with fill 51, every kept object's pixels are painted with that object's depth, the
// contributions are combined by a minimum and what exceeds max_depth becomes 0.
//
// A mask pixel is the label-file line index of its object, one byte (ids above 255 are stored as 255: only 0..63 can match a line).
// The depths come from the label encoder's per-line table (kitti_labels.hip, DEPTHS): line_depth[b][0][i] for the own file's line i,
// [b][1][i] for the partner's, +inf for a dropped or absent line.  A pixel is therefore two byte gathers and two table lookups.
//
// Pillow's Image.transform(AFFINE, NEAREST) has three code paths and real batches reach all of them: an 8-bit mask (mode L) takes
// the scale or the fixed path by its matrix (get_affine_transform leaves off-diagonal terms of exactly 0 or of about 1e-17), a 16-bit
// mask (mode I;16, what Image.fromarray makes of cv2.imread's uint16 array) always takes the generic one.  With a[0..5] the matrix,
// (w, h) the source and (W, H) the output:
//   scale path (a[1] == 0 and a[3] == 0; ImagingScaleAffine): xo = a[2] + a[0] * 0.5; for x = 0 .. W-1: xin[x] = xo < 0 ? -1 : (int)xo,
//     xo += a[0] - a RUNNING double sum, not x * a[0]; rows likewise with a[5], a[4].  The sums are sequential, so a small launch ahead
//     of the map kernel computes every image's xin[W] and yin[H] once, with exactly this order of additions.
//   fixed path (anything else, sides below 32768; affine_fixed): 16.16 fixed point, FIX(v) = floor(v * 65536 + 0.5);
//     xin = (FIX(a[2] + a[0]/2 + a[1]/2) + y * FIX(a[1]) + x * FIX(a[0])) >> 16, yin likewise with a[5], a[3], a[4]; int32 arithmetic.
//   generic path (16-bit masks; ImagingGenericTransform with affine_transform and the 16-bit nearest filter): in double,
//     xin = COORD(a[0] * (x + 0.5) + a[1] * (y + 0.5) + a[2]), yin = COORD(a[3] * (x + 0.5) + a[4] * (y + 0.5) + a[5]),
//     COORD(v) = v < 0 ? -1 : (int)v, products and sums in that order.
// A source position outside the mask reads the fill, id 51.  The flip is a mirrored source column.
//
// The map kernel: a workgroup owns DM_ROWS output rows of one image; the image's 128 table entries sit in LDS; a thread owns runs of
// four consecutive output columns cut at 16-byte boundaries of the output, so every full run is one 16-byte store whatever W and the
// row's start are, and the ragged ends of a row go float by float.  No scratch, 512 bytes of LDS.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DM_ROWS = 4;     // output rows per workgroup
constexpr int DM_FILL = 51;    // Pillow's fillcolor in the reference
constexpr int DM_LINES = 64;   // table entries per source (label lines 0..63)

struct DmP {
  const unsigned char* const* mask;   // pointer mode: per-image mask / partner mask (mask2 may be NULL: no image has a partner)
  const unsigned char* const* mask2;
  const unsigned char* arena;         // arena mode (arena != NULL): mask of frame p at arena + mask_off[p], p from the draw table
  const int64_t* mask_off;
  const double* draws;
  int draw_w;
  const unsigned char* wide;          // 16-bit source files: (B, 2) own | partner in pointer mode, (N) per frame in arena mode; NULL: none
  const int* hw;                      // (B, 2) source (h, w)
  const int* flip;                    // (B)
  const double* trans_inv;            // (B, 6)
  const float* line_depth;            // (B, 2, 64)
  int* xy;                            // (B, W + H) xin | yin of the scale path
  int B, H, W;
  float thr;                          // values above it become 0
};

__device__ __forceinline__ bool scale_path(const double* a) { return a[1] == 0.0 && a[3] == 0.0; }

// ---- the running sums of the scale path: wave 0 lane 0 walks the columns, wave 1 lane 0 the rows ----------------------------------
__global__ __launch_bounds__(128) void kitti_depth_index_kernel(DmP p) {
  const int b = blockIdx.x, wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) != 0) return;
  const double* a = p.trans_inv + (size_t)b * 6;
  if (!scale_path(a)) return;
  int* tab = p.xy + (size_t)b * (p.W + p.H) + (wave == 0 ? 0 : p.W);
  const int n = wave == 0 ? p.W : p.H;
  const double step = wave == 0 ? a[0] : a[4];
  double o = (wave == 0 ? a[2] : a[5]) + step * 0.5;
  for (int i = 0; i < n; ++i) {
    tab[i] = o < 0.0 ? -1 : (int)o;
    o += step;
  }
}

__device__ __forceinline__ int fix16(double v) { return (int)floor(v * 65536.0 + 0.5); }

// per-image constants of the warp, the same in every thread of a workgroup
struct Warp {
  const unsigned char *m0, *m1;
  const int *xin, *yin;
  const double* a;
  int h, w, flip, scale, wide0, wide1;
  unsigned a0, a1, a2, a3, a4, a5;  // the fixed path's integers (unsigned: products and sums wrap as Pillow's int arithmetic does)
};

__device__ __forceinline__ int coord(double v) { return v < 0.0 ? -1 : (int)v; }

// the id under output pixel (x, y) of a mask that is `wide` (a 16-bit file) or not; the fill outside
__device__ __forceinline__ int source_id(const Warp& Wp, const unsigned char* m, int wide, int x, int y) {
  int xs, ys;
  if (wide) {
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    xs = coord(Wp.a[0] * xc + Wp.a[1] * yc + Wp.a[2]);
    ys = coord(Wp.a[3] * xc + Wp.a[4] * yc + Wp.a[5]);
  } else if (Wp.scale) {
    xs = Wp.xin[x];
    ys = Wp.yin[y];
  } else {
    xs = (int)(Wp.a2 + (unsigned)y * Wp.a1 + (unsigned)x * Wp.a0) >> 16;
    ys = (int)(Wp.a5 + (unsigned)y * Wp.a4 + (unsigned)x * Wp.a3) >> 16;
  }
  if (xs < 0 || xs >= Wp.w || ys < 0 || ys >= Wp.h) return DM_FILL;
  return m[(size_t)ys * Wp.w + (Wp.flip ? Wp.w - 1 - xs : xs)];
}

__device__ __forceinline__ float paint(const Warp& Wp, const float* T, int x, int y, float thr) {
  const int id0 = source_id(Wp, Wp.m0, Wp.wide0, x, y);
  const int id1 = Wp.m1 != nullptr ? source_id(Wp, Wp.m1, Wp.wide1, x, y) : DM_FILL;
  float v = id0 < DM_LINES ? T[id0] : INFINITY;
  if (Wp.m1 != nullptr && id1 < DM_LINES) v = fminf(v, T[DM_LINES + id1]);
  return (v > thr || v == INFINITY) ? 0.f : v;
}

__global__ __launch_bounds__(256) void kitti_depth_map_kernel(DmP p, float* __restrict__ out) {
  __shared__ float T[2 * DM_LINES];
  const int b = blockIdx.y, y0 = blockIdx.x * DM_ROWS, tid = threadIdx.x;
  if (tid < 2 * DM_LINES) T[tid] = p.line_depth[(size_t)b * 2 * DM_LINES + tid];
  const double* a = p.trans_inv + (size_t)b * 6;
  Warp Wp;
  if (p.arena != nullptr) {
    const double* d = p.draws + (size_t)b * p.draw_w;
    const int pos = (int)d[0], par = (int)d[1];
    Wp.m0 = p.arena + p.mask_off[pos];
    Wp.m1 = par >= 0 ? p.arena + p.mask_off[par] : nullptr;
    Wp.wide0 = p.wide != nullptr && p.wide[pos] != 0;
    Wp.wide1 = p.wide != nullptr && par >= 0 && p.wide[par] != 0;
  } else {
    Wp.m0 = p.mask[b];
    Wp.m1 = p.mask2 != nullptr ? p.mask2[b] : nullptr;
    Wp.wide0 = p.wide != nullptr && p.wide[b * 2] != 0;
    Wp.wide1 = p.wide != nullptr && p.wide[b * 2 + 1] != 0;
  }
  Wp.a = a;
  Wp.h = p.hw[b * 2];
  Wp.w = p.hw[b * 2 + 1];
  Wp.flip = p.flip[b] != 0;
  Wp.scale = scale_path(a);
  Wp.xin = p.xy + (size_t)b * (p.W + p.H);
  Wp.yin = Wp.xin + p.W;
  Wp.a0 = (unsigned)fix16(a[0]);
  Wp.a1 = (unsigned)fix16(a[1]);
  Wp.a3 = (unsigned)fix16(a[3]);
  Wp.a4 = (unsigned)fix16(a[4]);
  Wp.a2 = (unsigned)fix16(a[2] + a[0] * 0.5 + a[1] * 0.5);
  Wp.a5 = (unsigned)fix16(a[5] + a[3] * 0.5 + a[4] * 0.5);
  __syncthreads();
  const int W = p.W, H = p.H;
  const int nq = (W + 6) / 4;  // runs per row, at most: a row that starts 3 floats behind a 16-byte boundary
  const int rows = min(DM_ROWS, H - y0);
  for (int q = tid; q < rows * nq; q += 256) {
    const int r = q / nq, k = q - r * nq, y = y0 + r;
    float* row = out + ((size_t)b * H + y) * W;
    const int mis = (int)(((uintptr_t)row >> 2) & 3);  // floats between the 16-byte boundary ahead of the row and its start
    const int lo = 4 * k - mis;
    if (lo >= W) continue;
    if (lo >= 0 && lo + 4 <= W) {
      float4 v;
      v.x = paint(Wp, T, lo, y, p.thr);
      v.y = paint(Wp, T, lo + 1, y, p.thr);
      v.z = paint(Wp, T, lo + 2, y, p.thr);
      v.w = paint(Wp, T, lo + 3, y, p.thr);
      *reinterpret_cast<float4*>(row + lo) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (lo + j >= 0 && lo + j < W) row[lo + j] = paint(Wp, T, lo + j, y, p.thr);
    }
  }
}

}  // namespace

extern "C" {

int y3d_kitti_depth_map(const unsigned char* const* mask, const unsigned char* const* mask2, const unsigned char* arena, const int64_t* mask_off,
                        const double* draws, int draw_w, const unsigned char* wide, const int* hw, const int* flip, const double* trans_inv,
                        const float* line_depth, int B, int out_h, int out_w, int max_side, double max_depth, int* xy, float* out,
                        void* stream) {
  Y3D_CHECK(B >= 1, "kitti_depth_map: B = %d", B);
  Y3D_CHECK(out_w >= 1 && out_h >= 1, "kitti_depth_map: bad resolution %d x %d", out_w, out_h);
  Y3D_CHECK(out_w < 32768 && out_h < 32768 && max_side >= 1 && max_side < 32768,
            "kitti_depth_map: a frame side of 32768 or more leaves Pillow's fixed-point path (output %d x %d, largest mask side %d)", out_w, out_h, max_side);
  Y3D_CHECK(hw && flip && trans_inv && line_depth && xy && out, "kitti_depth_map: null argument");
  Y3D_CHECK((arena != nullptr) != (mask != nullptr), "kitti_depth_map: either per-image mask pointers or an arena");
  Y3D_CHECK(arena == nullptr || (mask_off != nullptr && draws != nullptr && draw_w >= 2 && mask2 == nullptr),
            "kitti_depth_map: the arena needs its offsets and the draw table (position, partner)");
  Y3D_CHECK(((uintptr_t)out & 3) == 0, "kitti_depth_map: misaligned output");
  // the smallest float32 not below max_depth: a kept depth (<= max_depth in float64) never exceeds it once rounded to float32
  float thr = (float)max_depth;
  if ((double)thr < max_depth) thr = nextafterf(thr, INFINITY);
  DmP p{mask, mask2, arena, mask_off, draws, draw_w, wide, hw, flip, trans_inv, line_depth, xy, B, out_h, out_w, thr};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kitti_depth_index_kernel, dim3(B), dim3(128), 0, st, p);
  hipLaunchKernelGGL(kitti_depth_map_kernel, dim3(cdiv(out_h, DM_ROWS), B), dim3(256), 0, st, p, out);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
