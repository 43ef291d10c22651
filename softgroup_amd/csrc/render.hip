// render.hip -- result clouds to images: a z-buffered point splat over several views at once (sg_render_rasterize) and
// the colour lookup with optional eye-dome lighting (sg_render_shade).  The rules are stated in
// include/softgroup_hip.h; the reference has no counterpart.
//
// A z-buffer is a minimum over integer keys: key = (ord32(depth) << 32) | point, ord32 the order-preserving map of
// the float32 bits (the 32-bit form of obj_key in objects.hip).  The pixel's owner is the smallest key -- the nearest
// depth after rounding to float32, the LOWEST point among equal depths -- whatever the order of arrival, so two calls
// give the same bytes.  No float atomics; every double operation is rounded once (-ffp-contract=off) and the device
// evaluates no transcendental function: the cameras come from the host as a table of doubles.
//
// fill: the key buffer [V, H, W] is set to all ones (empty).  splat: a lane per point, the views in an inner loop
// (uniform per wave: the camera rows are read at uniform addresses); per covered pixel an 8-byte relaxed agent-scope
// load of the current key and a 64-bit atomicMin only when the new key is smaller (the key only ever falls: a stale
// read costs one extra atomic, never a wrong result).  The grid is capped at kRenderMaxBlocks and walked by a stride
// loop.  resolve: a lane per pixel turns keys into index / depth with plain coalesced stores.  shade: a lane per
// pixel, a gather of colors[index] (never dereferenced outside 0 .. n_colors-1: a flag instead).
//
// Every loop is bounded by an argument or by kRenderMaxRadius, every pixel and point index is checked before it
// addresses anything, no double is converted to an integer before its range test, no workgroup waits for another.
#include "common.h"

namespace sg {

constexpr int kRenderBlock = 256;
constexpr int kRenderMaxBlocks = 2048;                // grid cap of the splat kernel, walked by a stride loop
constexpr int kRenderMaxRadius = 16;                  // splat radius in pixels: at most 33 x 33 pixels per point
constexpr int kRenderMaxViews = 16;
constexpr int kRenderMaxSide = 8192;
constexpr int64_t kRenderMaxPixels = 1LL << 26;       // V * H * W
constexpr int kRenderCam = SG_RENDER_CAMERA_DOUBLES;  // doubles per camera row
constexpr uint64_t kRenderEmpty = ~0ULL;
constexpr double kRenderWindow = 1073741824.0;        // 2^30: u and v outside (-2^30, 2^30) cull the point

// float32 -> uint32 key with the same order (negative: all bits flipped; otherwise: sign bit set)
__device__ __forceinline__ uint32_t render_ord32(float d) {
  const uint32_t u = __float_as_uint(d);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float render_ord32_decode(uint32_t k) {
  return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

struct RsArgs {
  const float *coords;                  // [n, 3]
  const double *cams;                   // [n_views, kRenderCam]
  uint64_t *keys;                       // [n_views, height, width]
  int32_t *culled;                      // [n_views]
  int64_t n;
  int n_views, width, height, point_size;
  double world_radius;                  // > 0: the radius comes from the depth; else point_size
};

__global__ void __launch_bounds__(kRenderBlock) render_splat_kernel(RsArgs a) {
  __shared__ int s_culled[kRenderMaxViews];
  const int tid = threadIdx.x;
  if (tid < kRenderMaxViews) s_culled[tid] = 0;
  __syncthreads();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRenderBlock;
  const int64_t plane = static_cast<int64_t>(a.width) * a.height;
  // (the trip count is the same for every lane of a block: the camera rows stay at uniform addresses)
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kRenderBlock; base < a.n; base += stride) {
    const int64_t i = base + tid;
    const bool live = i < a.n;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) {
      x = static_cast<double>(a.coords[3 * i]), y = static_cast<double>(a.coords[3 * i + 1]);
      z = static_cast<double>(a.coords[3 * i + 2]);
    }
    for (int v = 0; v < a.n_views; ++v) {
      const double *c = a.cams + static_cast<int64_t>(v) * kRenderCam;            // (uniform address)
      const bool ortho = c[0] != 0.0;
      const double dx = x - c[1], dy = y - c[2], dz = z - c[3];
      const double xc = (c[4] * dx + c[5] * dy) + c[6] * dz;
      const double yc = (c[7] * dx + c[8] * dy) + c[9] * dz;
      const double zc = (c[10] * dx + c[11] * dy) + c[12] * dz;
      const double f = c[13];
      bool vis = true;                                                            // (a comparison with NaN is false)
      if (c[16] != 0.0) vis = zc >= c[17];
      if (c[18] != 0.0) vis = vis && zc <= c[19];
      double pu, pv;
      if (ortho) {
        pu = c[14] + f * xc, pv = c[15] - f * yc;
      } else {
        pu = c[14] + f * (xc / zc), pv = c[15] - f * (yc / zc);
      }
      vis = vis && pu > -kRenderWindow && pu < kRenderWindow && pv > -kRenderWindow && pv < kRenderWindow;
      if (live && !vis) atomicAdd(&s_culled[v], 1);                               // (LDS; one global add per block)
      if (!(live && vis)) continue;
      const int px = static_cast<int>(floor(pu)), py = static_cast<int>(floor(pv));   // |pu|, |pv| < 2^30
      int r = a.point_size;
      if (a.world_radius > 0.0) {
        const double rd = ortho ? floor(f * a.world_radius) : floor(f * (a.world_radius / zc));
        r = rd >= static_cast<double>(kRenderMaxRadius) ? kRenderMaxRadius : (rd >= 0.0 ? static_cast<int>(rd) : 0);
      }
      r = r < 0 ? 0 : (r > kRenderMaxRadius ? kRenderMaxRadius : r);
      const float d = static_cast<float>(zc) + 0.0f;
      const uint64_t key = (static_cast<uint64_t>(render_ord32(d)) << 32) | static_cast<uint64_t>(static_cast<uint32_t>(i));
      // the clipped splat: at most (2 r + 1)^2 <= 33 x 33 pixels, every one inside the image
      const int x0 = px - r < 0 ? 0 : px - r, x1 = px + r > a.width - 1 ? a.width - 1 : px + r;
      const int y0 = py - r < 0 ? 0 : py - r, y1 = py + r > a.height - 1 ? a.height - 1 : py + r;
      uint64_t *view = a.keys + static_cast<int64_t>(v) * plane;
      for (int yy = y0; yy <= y1; ++yy) {
        uint64_t *row = view + static_cast<int64_t>(yy) * a.width;
        for (int xx = x0; xx <= x1; ++xx) {
          const uint64_t seen = __hip_atomic_load(&row[xx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (key < seen) atomicMin(reinterpret_cast<unsigned long long *>(&row[xx]), static_cast<unsigned long long>(key));
        }
      }
    }
  }
  __syncthreads();
  if (tid < a.n_views && s_culled[tid]) atomicAdd(&a.culled[tid], s_culled[tid]);
}

__global__ void __launch_bounds__(kRenderBlock) render_resolve_kernel(const uint64_t *__restrict__ keys, int64_t pixels,
                                                                      int32_t *__restrict__ index,
                                                                      float *__restrict__ depth) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRenderBlock;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kRenderBlock + threadIdx.x; p < pixels; p += stride) {
    const uint64_t k = keys[p];
    const bool empty = k == kRenderEmpty;
    index[p] = empty ? -1 : static_cast<int32_t>(static_cast<uint32_t>(k));
    depth[p] = empty ? INFINITY : render_ord32_decode(static_cast<uint32_t>(k >> 32));
  }
}

struct ShArgs {
  const int32_t *index;                 // [n_views, height, width]
  const float *depth;
  const uint8_t *colors;                // [n_colors, 3]
  uint8_t *image;                       // [n_views, height, width, 3]
  int32_t *flags;
  int64_t n_colors;
  int n_views, width, height;
  int bg[3];
  int edl, radius;
  double strength, scale;
};

// the eight neighbours of eye-dome lighting in the order of the header, in units of the radius
__constant__ int kEdlDx[8] = {-1, 1, 0, 0, -1, 1, -1, 1};
__constant__ int kEdlDy[8] = {0, 0, -1, 1, -1, -1, 1, 1};

__global__ void __launch_bounds__(kRenderBlock) render_shade_kernel(ShArgs a) {
  const int64_t plane = static_cast<int64_t>(a.width) * a.height;
  const int64_t pixels = plane * a.n_views;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRenderBlock;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kRenderBlock + threadIdx.x; p < pixels; p += stride) {
    const int32_t i = a.index[p];
    int c0 = a.bg[0], c1 = a.bg[1], c2 = a.bg[2];
    if (i >= 0) {
      if (static_cast<int64_t>(i) >= a.n_colors) {
        atomicOr(a.flags, SG_RENDER_FLAG_COLOR_INDEX);
      } else {
        c0 = a.colors[3 * static_cast<int64_t>(i)], c1 = a.colors[3 * static_cast<int64_t>(i) + 1];
        c2 = a.colors[3 * static_cast<int64_t>(i) + 2];
        if (a.edl) {
          const int64_t q = p % plane;
          const int py = static_cast<int>(q / a.width), px = static_cast<int>(q - static_cast<int64_t>(py) * a.width);
          const double d = static_cast<double>(a.depth[p]);
          double sum = 0.0;
          int count = 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int nx = px + kEdlDx[k] * a.radius, ny = py + kEdlDy[k] * a.radius;
            if (nx < 0 || nx >= a.width || ny < 0 || ny >= a.height) continue;
            ++count;
            const int64_t pn = p + static_cast<int64_t>(ny - py) * a.width + (nx - px);
            if (a.index[pn] < 0) continue;                                    // (an empty neighbour contributes 0)
            double t = d - static_cast<double>(a.depth[pn]);
            t = t > 0.0 ? t : 0.0;
            t = t / a.scale;
            t = t < 1.0 ? t : 1.0;
            sum = sum + t;
          }
          const double resp = count ? sum / static_cast<double>(count) : 0.0;
          const double shade = 1.0 / (1.0 + a.strength * resp);
          c0 = static_cast<int>(floor(static_cast<double>(c0) * shade + 0.5));
          c1 = static_cast<int>(floor(static_cast<double>(c1) * shade + 0.5));
          c2 = static_cast<int>(floor(static_cast<double>(c2) * shade + 0.5));
        }
      }
    }
    uint8_t *out = a.image + 3 * p;
    out[0] = static_cast<uint8_t>(c0), out[1] = static_cast<uint8_t>(c1), out[2] = static_cast<uint8_t>(c2);
  }
}

static bool render_range(const char *who, int64_t n, int n_views, int width, int height) {
  if (n < 0 || n >= (1LL << 31) - 1 || n_views < 1 || n_views > kRenderMaxViews || width < 1 || width > kRenderMaxSide ||
      height < 1 || height > kRenderMaxSide ||
      static_cast<int64_t>(n_views) * width * height > kRenderMaxPixels) {
    set_error("%s: %lld points into %d views of %d x %d outside the supported range (< 2^31 - 1 points, 1 .. %d views, "
              "sides 1 .. %d, at most 2^26 pixels)", who, static_cast<long long>(n), n_views, width, height,
              kRenderMaxViews, kRenderMaxSide);
    return false;
  }
  return true;
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_render_rasterize_workspace_bytes(int n_views, int width, int height) {
  if (n_views < 1 || width < 1 || height < 1) return 0;
  return align_up(sizeof(uint64_t) * static_cast<size_t>(n_views) * static_cast<size_t>(width) *
                  static_cast<size_t>(height)) + 256;
}

int sg_render_rasterize(const float *coords, int64_t n, const double *cams, int n_views, int width, int height,
                        int point_size, double world_radius, int stages, int32_t *index, float *depth,
                        int32_t *culled, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!render_range("sg_render_rasterize", n, n_views, width, height)) return SG_ERR_UNSUPPORTED;
  SG_REQUIRE(world_radius > 0.0 || (point_size >= 0 && point_size <= kRenderMaxRadius),
             "sg_render_rasterize: point_size %d (0 .. %d) without a world radius > 0", point_size, kRenderMaxRadius);
  SG_REQUIRE(!(world_radius != world_radius), "sg_render_rasterize: the world radius is NaN");
  SG_REQUIRE(cams != nullptr && index != nullptr && depth != nullptr && culled != nullptr &&
                 (n == 0 || coords != nullptr), "sg_render_rasterize: null array");
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_render_rasterize_workspace_bytes(n_views, width, height),
             "sg_render_rasterize: workspace of %zu bytes, %zu needed", ws_bytes,
             sg_render_rasterize_workspace_bytes(n_views, width, height));
  hipStream_t stream = as_stream(stream_);
  const int64_t pixels = static_cast<int64_t>(n_views) * width * height;
  Workspace wsp(ws, ws_bytes);
  uint64_t *keys = wsp.take<uint64_t>(static_cast<size_t>(pixels));
  SG_REQUIRE(keys != nullptr, "sg_render_rasterize: workspace too small");
  if (stages & SG_RENDER_STAGE_FILL) {
    if (hipMemsetAsync(culled, 0, sizeof(int32_t) * n_views, stream) != hipSuccess)
      return check_launch("sg_render_rasterize (memset)");
    FillList fl;
    fl.add(keys, sizeof(uint64_t) * static_cast<size_t>(pixels), 0xff);
    fill_many(fl, stream);
  }
  if ((stages & SG_RENDER_STAGE_SPLAT) && n > 0) {
    RsArgs a;
    a.coords = coords, a.cams = cams, a.keys = keys, a.culled = culled, a.n = n, a.n_views = n_views;
    a.width = width, a.height = height, a.point_size = world_radius > 0.0 ? 0 : point_size;
    a.world_radius = world_radius > 0.0 ? world_radius : 0.0;
    render_splat_kernel<<<grid_for(n, kRenderBlock, kRenderMaxBlocks), kRenderBlock, 0, stream>>>(a);
  }
  if (stages & SG_RENDER_STAGE_RESOLVE)
    render_resolve_kernel<<<grid_for(pixels, kRenderBlock, kRenderMaxBlocks), kRenderBlock, 0, stream>>>(keys, pixels,
                                                                                                        index, depth);
  return check_launch("sg_render_rasterize");
}

int sg_render_shade(const int32_t *index, const float *depth, int n_views, int width, int height,
                    const uint8_t *colors, int64_t n_colors, int bg_r, int bg_g, int bg_b, int edl, double strength,
                    int radius, double scale, uint8_t *image, int32_t *flags, sg_stream_t stream_) {
  if (!render_range("sg_render_shade", 0, n_views, width, height)) return SG_ERR_UNSUPPORTED;
  SG_REQUIRE(n_colors >= 0 && bg_r >= 0 && bg_r <= 255 && bg_g >= 0 && bg_g <= 255 && bg_b >= 0 && bg_b <= 255,
             "sg_render_shade: %lld colours, background (%d, %d, %d): counts >= 0, components 0 .. 255",
             static_cast<long long>(n_colors), bg_r, bg_g, bg_b);
  SG_REQUIRE(!edl || (strength >= 0.0 && radius >= 1 && radius <= 4 && scale > 0.0),
             "sg_render_shade: eye-dome lighting wants strength >= 0, a radius of 1 .. 4 pixels and a scale > 0");
  SG_REQUIRE(index != nullptr && image != nullptr && flags != nullptr && (!edl || depth != nullptr) &&
                 (n_colors == 0 || colors != nullptr), "sg_render_shade: null array");
  hipStream_t stream = as_stream(stream_);
  if (hipMemsetAsync(flags, 0, sizeof(int32_t), stream) != hipSuccess) return check_launch("sg_render_shade (memset)");
  ShArgs a;
  a.index = index, a.depth = depth, a.colors = colors, a.image = image, a.flags = flags, a.n_colors = n_colors;
  a.n_views = n_views, a.width = width, a.height = height, a.bg[0] = bg_r, a.bg[1] = bg_g, a.bg[2] = bg_b;
  a.edl = edl != 0, a.radius = edl ? radius : 1, a.strength = edl ? strength : 0.0, a.scale = edl ? scale : 1.0;
  const int64_t pixels = static_cast<int64_t>(n_views) * width * height;
  render_shade_kernel<<<grid_for(pixels, kRenderBlock, kRenderMaxBlocks), kRenderBlock, 0, stream>>>(a);
  return check_launch("sg_render_shade");
}

}  // extern "C"
