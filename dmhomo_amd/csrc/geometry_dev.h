// Per-pixel device functions of the geometry kernels, shared by geometry.hip (G2 homography flow, G3 flow_to_image, G4 flow_warp),
// preview.hip (the preview sheets fuse G3 and G4; the homography warp) and relabel.hip (which fuses G2, G3 and the homography
// warp): one definition, so the fused outputs are bit for bit what the stand-alone kernels write.
// They mirror the reference's op order where integers come out (grid-sample corner indices): no FMA contraction here.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

// G2: get_flow_np DDP:954-967 for one pixel: h . (x, y, 1) in float64 on the integer grid, w' + 1e-6 (DDP:958-959), the
// subtraction in float64, then the cast.  h: nine doubles, row-major (global memory or LDS)
__device__ __forceinline__ void homography_flow_pixel(const double* __restrict__ h, int xi, int yi, float& u, float& v) {
  const double x = (double)xi, y = (double)yi;
  const double qx = h[0] * x + h[1] * y + h[2];
  const double qy = h[3] * x + h[4] * y + h[5];
  const double qw = (h[6] * x + h[7] * y + h[8]) + 1e-6;
  u = (float)(qx / qw - x);
  v = (float)(qy / qw - y);
}

// G3: flow_to_image DDP:1479-1485 + matplotlib.colors.hsv_to_rgb for one pixel
__device__ __forceinline__ void flow_pixel_to_rgb(float u, float v, float max_flow, float& r, float& g, float& bl) {
  const float n = 8.f;
  const float mag = sqrtf(u * u + v * v);
  const float ang = atan2f(v, u);
  float hh = fmodf(ang / 6.283185307179586f + 1.f, 1.f);  // np.mod(angle / (2 pi) + 1, 1), operand >= 0.5
  float ss = fminf(fmaxf(mag * n / max_flow, 0.f), 1.f);
  float vv = fminf(fmaxf(n - ss, 0.f), 1.f);
  // matplotlib.colors.hsv_to_rgb: i = (h*6).astype(int); f = h*6 - i is float64 there (f32 - int64),
  // so q and t are formed in f64 and rounded to fp32 on store; p stays fp32.
  const float h6 = hh * 6.0f;
  const int i = (int)h6;
  const double f = (double)h6 - (double)i;
  const float pp = vv * (1.0f - ss);
  const float qq = (float)((double)vv * (1.0 - (double)ss * f));
  const float tt = (float)((double)vv * (1.0 - (double)ss * (1.0 - f)));
  switch (i % 6) {
    case 0: r = vv; g = tt; bl = pp; break;
    case 1: r = qq; g = vv; bl = pp; break;
    case 2: r = pp; g = vv; bl = tt; break;
    case 3: r = pp; g = qq; bl = vv; break;
    case 4: r = tt; g = pp; bl = vv; break;
    default: r = vv; g = pp; bl = qq; break;
  }
  if (ss == 0.f) r = g = bl = vv;
}

// G4.  flow_warp = grid_sample(bilinear, border, align_corners=True) of torch's CPU kernel, for the pixel (xi, yi) moved by
// (fu, fv):
//   g  = 2.0*v/(W-1) - 1.0;  ix = (g+1)*((W-1)/2);  ix = min(W-1, max(ix, 0));  x0 = floor(ix)
//   w = ix-x0, e = (x0+1)-ix, n = iy-y0, s = (y0+1)-iy
//   out = fma(se, n*w, fma(sw, n*e, fma(ne, s*w, nw*(s*e))))
// The corner indices always lie inside the image (the coordinate is clipped); a corner one past the last row / column is
// read as 0 (its weight is 0 there).
struct FlowWarpTaps {
  int x0, y0, x1, y1;
  bool x1ok, y1ok;
  float wnw, wne, wsw, wse;
};
__device__ __forceinline__ FlowWarpTaps flow_warp_taps(float fu, float fv, int xi, int yi, int H, int W) {
  FlowWarpTaps t;
  const float vx = (float)xi + fu;
  const float vy = (float)yi + fv;
  const float gx = 2.0f * vx / (float)(W - 1) - 1.0f;
  const float gy = 2.0f * vy / (float)(H - 1) - 1.0f;
  float ix = (gx + 1.f) * ((float)(W - 1) / 2.f);
  float iy = (gy + 1.f) * ((float)(H - 1) / 2.f);
  ix = fminf((float)(W - 1), fmaxf(ix, 0.f));
  iy = fminf((float)(H - 1), fmaxf(iy, 0.f));
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  t.x0 = (int)fx0;
  t.y0 = (int)fy0;
  const float w = ix - fx0, e = (fx0 + 1.f) - ix, n = iy - fy0, s = (fy0 + 1.f) - iy;
  t.wnw = s * e;
  t.wne = s * w;
  t.wsw = n * e;
  t.wse = n * w;
  t.x1ok = t.x0 + 1 <= W - 1;
  t.y1ok = t.y0 + 1 <= H - 1;
  t.x1 = t.x1ok ? t.x0 + 1 : t.x0;
  t.y1 = t.y1ok ? t.y0 + 1 : t.y0;
  return t;
}
// one channel plane xc [H][W] sampled at the taps
__device__ __forceinline__ float flow_warp_sample(const float* __restrict__ xc, const FlowWarpTaps& t, int W) {
  const float nw = xc[(size_t)t.y0 * W + t.x0];
  const float ne = t.x1ok ? xc[(size_t)t.y0 * W + t.x1] : 0.f;
  const float sw = t.y1ok ? xc[(size_t)t.y1 * W + t.x0] : 0.f;
  const float se = (t.x1ok && t.y1ok) ? xc[(size_t)t.y1 * W + t.x1] : 0.f;
  float acc = nw * t.wnw;
  acc = fmaf(ne, t.wne, acc);
  acc = fmaf(sw, t.wsw, acc);
  acc = fmaf(se, t.wse, acc);
  return acc;
}

// HEM's homo_convert_to_flow (HEM/dataset/data_loader.py:42-52 over from_homography_to_pixel_wise_mapping,
// flow_and_mapping_operations.py:454-484, and convert_mapping_to_flow, :155-195) for one pixel: the mapping H.(x, y, 1) in
// float64 with the reference's epsilon 1e-8 on the divisor, rounded to fp32 (map.astype(float32)), minus the fp32 grid.
// Not G2 (dmh_homography_flow): that one is DDP's get_flow_np with 1e-6 and the subtraction in float64.
__device__ __forceinline__ void hem_flow_pixel(const double* __restrict__ Hm, int xi, int yi, float& u, float& v) {
  const double x = (double)xi, y = (double)yi;
  const double wq = (Hm[6] * x + Hm[7] * y) + Hm[8];
  const float mx = (float)(((Hm[0] * x + Hm[1] * y) + Hm[2]) / (wq + 1e-8));
  const float my = (float)(((Hm[3] * x + Hm[4] * y) + Hm[5]) / (wq + 1e-8));
  u = mx - (float)xi;
  v = my - (float)yi;
}

// The homography warp (preview.hip: homography_warp_kernel has the contract) in three pieces.
// 1. the inverse as adjugate times 1 / determinant: inv[k] = adj(m)[k] * (1 / det), zeros for a singular m (cv2.invert)
__device__ __forceinline__ void homography_inverse(const double* __restrict__ m, double* __restrict__ inv) {
  const double a0 = m[4] * m[8] - m[5] * m[7], a1 = m[2] * m[7] - m[1] * m[8], a2 = m[1] * m[5] - m[2] * m[4];
  const double a3 = m[5] * m[6] - m[3] * m[8], a4 = m[0] * m[8] - m[2] * m[6], a5 = m[2] * m[3] - m[0] * m[5];
  const double a6 = m[3] * m[7] - m[4] * m[6], a7 = m[1] * m[6] - m[0] * m[7], a8 = m[0] * m[4] - m[1] * m[3];
  const double det = m[0] * a0 + m[1] * a3 + m[2] * a6;
  const double id = det != 0.0 ? 1.0 / det : 0.0;
  inv[0] = a0 * id, inv[1] = a1 * id, inv[2] = a2 * id;
  inv[3] = a3 * id, inv[4] = a4 * id, inv[5] = a5 * id;
  inv[6] = a6 * id, inv[7] = a7 * id, inv[8] = a8 * id;
}
// 2. the source coordinate inv . (x, y, 1) of the destination pixel (xi, yi)  (cv2: w ? 1 / w : 0)
__device__ __forceinline__ void homography_warp_source(const double* __restrict__ inv, int xi, int yi, double& sx, double& sy) {
  const double x = (double)xi, y = (double)yi;
  const double qx = inv[0] * x + inv[1] * y + inv[2];
  const double qy = inv[3] * x + inv[4] * y + inv[5];
  const double qw = inv[6] * x + inv[7] * y + inv[8];
  sx = qw != 0.0 ? qx / qw : 0.0;
  sy = qw != 0.0 ? qy / qw : 0.0;
}
// 3. the exact bilinear sample of one channel plane sc [H][W] at (sx, sy) in float64, rounded once; every tap outside the image
// reads 0: a coordinate outside (-1, W) x (-1, H) (or NaN) has no tap inside
struct HomographyWarpTaps {
  bool any, xl, xr, yt, yb;
  int x0, y0;      // -1 .. W-1, -1 .. H-1
  double fx, fy;
};
__device__ __forceinline__ HomographyWarpTaps homography_warp_taps(double sx, double sy, int H, int W) {
  HomographyWarpTaps t;
  t.any = sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H;
  const double fx0 = floor(sx), fy0 = floor(sy);
  t.x0 = t.any ? (int)fx0 : 0;
  t.y0 = t.any ? (int)fy0 : 0;
  t.fx = sx - fx0;
  t.fy = sy - fy0;
  t.xl = t.x0 >= 0, t.xr = t.x0 + 1 <= W - 1, t.yt = t.y0 >= 0, t.yb = t.y0 + 1 <= H - 1;
  return t;
}
__device__ __forceinline__ float homography_warp_sample(const float* __restrict__ sc, const HomographyWarpTaps& t, int W) {
  if (!t.any) return 0.f;
  const double nw = (t.xl && t.yt) ? (double)sc[(size_t)t.y0 * W + t.x0] : 0.0;
  const double ne = (t.xr && t.yt) ? (double)sc[(size_t)t.y0 * W + t.x0 + 1] : 0.0;
  const double sw = (t.xl && t.yb) ? (double)sc[(size_t)(t.y0 + 1) * W + t.x0] : 0.0;
  const double se = (t.xr && t.yb) ? (double)sc[(size_t)(t.y0 + 1) * W + t.x0 + 1] : 0.0;
  return (float)((1.0 - t.fy) * ((1.0 - t.fx) * nw + t.fx * ne) + t.fy * ((1.0 - t.fx) * sw + t.fx * se));
}
