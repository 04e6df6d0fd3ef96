// Object removal: the background plate (include/mdqe_hip.h has the rule, above mdqe_plate_update_u8); tests/_plate_ref.py restates it in
// numpy and every comparison is exact.  The compositing painters take the plate's picture as their backdrop; no painter changes.
//
// STATE: int32 cells on the output grid, (P_0, P_1, P_2, n) for RGB, (P, n) for luma, (P_U, P_V, n, 0) for chroma; P in 24.8 fixed point.
//   update   one thread per cell, lanes along X: the cell comes in with one vector load, the thread walks the call's F frames in video
//            order -- a byte of `block` (coalesced along X) decides whether the frame's value (coalesced along X where the source has the
//            output's size) enters the running mean -- and the cell goes back with one vector store.  A surface call covers the luma
//            cells with its first blocks and the chroma cells with the rest: one launch.
//   picture  as grow.hip, a thread block owns a TILE of 16 x 64 cells of one plane: 256 threads, phases between barriers:
//            0 own      the tile's own counts: a tile without a never-seen cell sets no flag and goes straight to phase 3;
//            1 stage    the (16 + 2R) x (64 + 2R) neighbourhood's "seen" bits go into LDS as bytes, 0 outside the plane;
//            2 columns  per tile row and staged column the minimum over |dy| <= R of dy^2 << 8 | (dy + R) of the seen cells;
//            3 rows     one cell per thread and step: a seen cell shows (P + 128) >> 8; any other scans dx = -R .. R ascending for a
//                       strictly smaller dx^2 << 8 + that column's key, which is the definition's smallest (d2, Y', X'), reads that
//                       cell's P from the state, or takes the fill; single-sample stores at any alignment.
//            A surface call covers the luma tiles with its first blocks and the chroma tiles (reach (R + 1) / 2) with the rest.
// The LDS is static, 18.4 KB whatever the reach.  No data-dependent order, no atomics, no global scratch: identical from run to run.
#include "render_rule.h"

namespace {

constexpr int TH = 16, TW = 64;                  // the tile, in cells
constexpr int MAX_R = 32;
constexpr int PITCH = TW + 2 * MAX_R;            // cells between the rows of both LDS planes
constexpr uint32_t NONE = 0x40000000u;           // a column without a seen cell: NONE + (dx^2 << 8) stays below 2^31 and is never accepted

// n' = min(n + 1, N) is the caller's; P' = P + floordiv(256 * s - P + (n' >> 1), n')
__device__ __forceinline__ int learn(int P, int s, int n) {
  const int a = 256 * s - P + (n >> 1);
  int q = a / n;
  if (a % n < 0) --q;                            // (C++ rounds towards zero: one less where a negative quotient was cut)
  return P + q;
}

// ---- update ---------------------------------------------------------------------------------------------------------------------------
struct UpdateRgbArgs {
  RgbSource src;
  const unsigned char* block;    // [F, Ho, Wo]
  int4* state;                   // [Ho, Wo]
  int F, Ho, Wo, n_max, ident;
};

template <int KIND>
__global__ __launch_bounds__(256) void plate_update_rgb_kernel(const UpdateRgbArgs a) {
  const long cells = (long)a.Ho * a.Wo;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const int Y = (int)(i / a.Wo), X = (int)(i - (long)Y * a.Wo);
  int4 c = a.state[i];
  const int sy = a.ident ? Y : (int)((long)Y * a.src.h0 / a.Ho);
  const int sx = a.ident ? X : (int)((long)X * a.src.w0 / a.Wo);
  const long at = (long)sy * a.src.w0 + sx;
  for (int f = 0; f < a.F; ++f) {
    if (a.block[f * cells + i] != 0) continue;
    const uint32_t s = src_px<KIND>(a.src, f * a.src.frame_stride + at);
    const int n = c.w + 1 < a.n_max ? c.w + 1 : a.n_max;
    c.x = learn(c.x, (int)(s & 0xFFu), n);
    c.y = learn(c.y, (int)(s >> 8 & 0xFFu), n);
    c.z = learn(c.z, (int)(s >> 16), n);
    c.w = n;
  }
  a.state[i] = c;
}

struct UpdateYuvArgs {
  const unsigned char* y; long y_pitch, y_stride;
  const unsigned char* uv; long uv_pitch, uv_stride;
  const unsigned char* block;    // [F, H, W]
  int2* state_y;                 // [H, W]
  int4* state_c;                 // [ch, cw]
  int F, H, W, n_max;
  unsigned luma_blocks;          // blocks 0 .. luma_blocks - 1 own luma cells, the rest chroma cells
};

template <int FMT>
__device__ __forceinline__ int sample_at(const unsigned char* row, int i) {
  return (int)value_of<FMT>(row_raw<FMT>(row, i));
}

template <int FMT>
__global__ __launch_bounds__(256) void plate_update_yuv_kernel(const UpdateYuvArgs a) {
  const long cells = (long)a.H * a.W;
  if (blockIdx.x < a.luma_blocks) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const int Y = (int)(i / a.W), X = (int)(i - (long)Y * a.W);
    int2 c = a.state_y[i];
    for (int f = 0; f < a.F; ++f) {
      if (a.block[f * cells + i] != 0) continue;
      const int s = sample_at<FMT>(a.y + f * a.y_stride + Y * a.y_pitch, X);
      const int n = c.y + 1 < a.n_max ? c.y + 1 : a.n_max;
      c.x = learn(c.x, s, n);
      c.y = n;
    }
    a.state_y[i] = c;
    return;
  }
  const int ch = (a.H + 1) / 2, cw = (a.W + 1) / 2;
  const long i = (long)(blockIdx.x - a.luma_blocks) * 256 + threadIdx.x;
  if (i >= (long)ch * cw) return;
  const int Y = (int)(i / cw), X = (int)(i - (long)Y * cw);
  const bool right = 2 * X + 1 < a.W, below = 2 * Y + 1 < a.H;         // which of the block's other pixels lie in the picture
  int4 c = a.state_c[i];
  for (int f = 0; f < a.F; ++f) {
    const unsigned char* b = a.block + f * cells + (long)(2 * Y) * a.W + 2 * X;
    uint32_t any = b[0];
    if (right) any |= b[1];
    if (below) any |= b[a.W];
    if (right && below) any |= b[a.W + 1];
    if (any != 0) continue;
    const unsigned char* row = a.uv + f * a.uv_stride + Y * a.uv_pitch;
    const int n = c.z + 1 < a.n_max ? c.z + 1 : a.n_max;
    c.x = learn(c.x, sample_at<FMT>(row, 2 * X), n);
    c.y = learn(c.y, sample_at<FMT>(row, 2 * X + 1), n);
    c.z = n;
  }
  a.state_c[i] = c;
}

// ---- picture --------------------------------------------------------------------------------------------------------------------------
// A plane of state and where its picture goes.  KIND 0: RGB cells (P_0, P_1, P_2, n) -> bytes [h, w, 3]; 1: luma cells (P, n) -> samples
// [h, w]; 2: chroma cells (P_U, P_V, n, 0) -> sample pairs [h, 2 w].
struct PlaneArgs {
  const int* state;
  unsigned char* out;
  long pitch;                    // bytes between the output's rows
  int h, w, reach;
  unsigned tiles_x, tiles_y;
};

struct PictureArgs {
  PlaneArgs p[2];                // RGB: p[0]; a surface: luma, chroma
  const void* fill;              // uint8 [3] (RGB) or uint16 [3] (a surface)
  unsigned first_blocks;         // blocks 0 .. first_blocks - 1 own tiles of p[0], the rest tiles of p[1]
};

template <int KIND> struct Cell;
template <> struct Cell<0> { static constexpr int INTS = 4, CH = 3; };
template <> struct Cell<1> { static constexpr int INTS = 2, CH = 1; };
template <> struct Cell<2> { static constexpr int INTS = 4, CH = 2; };

// the cell at (Y, X) as (channels .., n) in v[0 .. CH]
template <int KIND>
__device__ __forceinline__ void load_cell(const PlaneArgs& a, int Y, int X, int* v) {
  const long i = (long)Y * a.w + X;
  if (Cell<KIND>::INTS == 4) {
    const int4 c = ((const int4*)a.state)[i];
    v[0] = c.x; v[1] = c.y; v[2] = c.z; v[3] = c.w;
  } else {
    const int2 c = ((const int2*)a.state)[i];
    v[0] = c.x; v[1] = c.y;
  }
}

template <int KIND>
__device__ __forceinline__ int count_at(const PlaneArgs& a, int Y, int X) {
  return a.state[((long)Y * a.w + X) * Cell<KIND>::INTS + Cell<KIND>::CH];
}

template <int KIND, int FMT>
__device__ __forceinline__ void put(const PlaneArgs& a, int Y, int X, const uint32_t* v) {
  unsigned char* row = a.out + Y * a.pitch;
  if (KIND == 0) {
    row[3 * X] = (unsigned char)v[0]; row[3 * X + 1] = (unsigned char)v[1]; row[3 * X + 2] = (unsigned char)v[2];
  } else if (KIND == 1) {
    row_put<FMT>(row, X, stored<FMT>(v[0]));
  } else {
    row_put<FMT>(row, 2 * X, stored<FMT>(v[0]));
    row_put<FMT>(row, 2 * X + 1, stored<FMT>(v[1]));
  }
}

template <int KIND, int FMT>
__device__ __forceinline__ void picture_tile(const PlaneArgs& a, const void* fill_ptr, unsigned b, unsigned char* s, uint32_t* col, int* flag) {
  constexpr int CH = Cell<KIND>::CH;
  const int tid = (int)threadIdx.x;
  const unsigned tx = b % a.tiles_x, ty = b / a.tiles_x;
  const int Y0 = (int)ty * TH, X0 = (int)tx * TW;
  const int th = a.h - Y0 < TH ? a.h - Y0 : TH, tw = a.w - X0 < TW ? a.w - X0 : TW;
  const int R = a.reach, SH = TH + 2 * R, SW = TW + 2 * R;
  if (tid == 0) *flag = 0;
  __syncthreads();
  for (int i = tid; i < th * TW; i += 256) {
    const int r = i / TW, c = i % TW;
    if (c < tw && count_at<KIND>(a, Y0 + r, X0 + c) == 0) *flag = 1;
  }
  __syncthreads();
  const bool search = *flag != 0 && R > 0;                            // (uniform over the block; reach 0: a never-seen cell has no candidate)
  if (search) {
    for (int r = tid >> 7; r < SH; r += 2) {                          // (SW <= 128)
      const int c = tid & 127;
      if (c >= SW) continue;
      const int Y = Y0 - R + r, X = X0 - R + c;
      unsigned char v = 0;
      if (Y >= 0 && Y < a.h && X >= 0 && X < a.w) v = count_at<KIND>(a, Y, X) > 0 ? 1 : 0;
      s[r * PITCH + c] = v;
    }
    __syncthreads();
    for (int i = tid; i < th * SW; i += 256) {
      const int r = i / SW, c = i - r * SW;
      const unsigned char* q = s + (r + R) * PITCH + c;
      uint32_t best = NONE;
#pragma unroll 4
      for (int dy = -R; dy <= R; ++dy) {
        const uint32_t key = (uint32_t)(dy * dy) << 8 | (uint32_t)(dy + R);
        best = q[dy * PITCH] != 0 && key < best ? key : best;
      }
      col[r * PITCH + c] = best;
    }
    __syncthreads();
  }
  uint32_t fill[3];
  if (KIND == 0) {
    for (int k = 0; k < 3; ++k) fill[k] = ((const unsigned char*)fill_ptr)[k];
  } else {
    const unsigned short* f = (const unsigned short*)fill_ptr;
    const uint32_t mask = FMT ? 0x3FFu : 0xFFu;
    fill[0] = (KIND == 1 ? f[0] : f[1]) & mask;
    fill[1] = f[2] & mask;
    fill[2] = 0u;
  }
  const uint32_t r2 = (uint32_t)(R * R);
  for (int i = tid; i < th * TW; i += 256) {
    const int r = i / TW, c = i % TW;
    if (c >= tw) continue;
    const int Y = Y0 + r, X = X0 + c;
    int v[4];
    load_cell<KIND>(a, Y, X, v);
    uint32_t o[3] = {fill[0], fill[1], fill[2]};
    bool seen = v[CH] > 0;
    if (!seen && search) {
      const uint32_t* q = col + r * PITCH + c + R;
      uint32_t best = NONE;
      int at = 0;
#pragma unroll 4
      for (int dx = -R; dx <= R; ++dx) {
        const uint32_t key = q[dx] + ((uint32_t)(dx * dx) << 8);
        at = key < best ? dx : at;
        best = key < best ? key : best;
      }
      if ((best >> 8) <= r2) {                                        // (a seen cell: inside the plane)
        load_cell<KIND>(a, Y + (int)(best & 0xFFu) - R, X + at, v);
        seen = true;
      }
    }
    if (seen)
      for (int k = 0; k < CH; ++k) o[k] = (uint32_t)(v[k] + 128) >> 8;
    put<KIND, FMT>(a, Y, X, o);
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void plate_picture_kernel(const PictureArgs a, const int rgb) {
  __shared__ unsigned char s[(TH + 2 * MAX_R) * PITCH];               // the neighbourhood: 1 where the cell has been seen
  __shared__ uint32_t col[TH * PITCH];                                // per tile row and staged column: min (dy^2 << 8 | dy + R), or NONE
  __shared__ int flag;
  if (rgb) picture_tile<0, 0>(a.p[0], a.fill, blockIdx.x, s, col, &flag);
  else if (blockIdx.x < a.first_blocks) picture_tile<1, FMT>(a.p[0], a.fill, blockIdx.x, s, col, &flag);
  else picture_tile<2, FMT>(a.p[1], a.fill, blockIdx.x - a.first_blocks, s, col, &flag);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// [p, p + n) and [q, q + m) share a byte
inline bool meet(const void* p, long n, const void* q, long m) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return n > 0 && m > 0 && a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

inline PlaneArgs plane(const int* state, void* out, long pitch, int h, int w, int reach) {
  PlaneArgs p;
  p.state = state; p.out = (unsigned char*)out; p.pitch = pitch;
  p.h = h; p.w = w; p.reach = reach;
  p.tiles_x = (unsigned)((w + TW - 1) / TW);
  p.tiles_y = (unsigned)((h + TH - 1) / TH);
  return p;
}

}  // namespace

extern "C" int mdqe_plate_update_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                                    const unsigned char* block, int F, int Ho, int Wo, int n_max, int* plate, void* stream) {
  MDQE_REQUIRE(n_max >= 1 && n_max <= 256);
  MDQE_REQUIRE(F >= 0 && Ho >= 0 && Wo >= 0);
  MDQE_REQUIRE((long)Ho * Wo * 4 < 0x7FFFFFFFL && (long)F * Ho * Wo < 0x7FFFFFFFL);
  MDQE_REQUIRE(h0 >= 1 && w0 >= 1 && (long)h0 * Ho < 0x7FFFFFFFL && (long)w0 * Wo < 0x7FFFFFFFL);
  MDQE_REQUIRE(frame_stride >= 3L * h0 * w0);
  const long cells = (long)Ho * Wo;
  if (F == 0 || cells == 0) return MDQE_OK;
  MDQE_REQUIRE(frames != nullptr && block != nullptr && plate != nullptr);
  MDQE_REQUIRE(((uintptr_t)plate & 15u) == 0);
  const long esz = is_u8 ? 1 : 4;
  MDQE_REQUIRE(is_u8 || ((uintptr_t)frames & 3u) == 0);
  MDQE_REQUIRE(!meet(plate, cells * 16, frames, ((F - 1) * frame_stride + 3L * h0 * w0) * esz));
  MDQE_REQUIRE(!meet(plate, cells * 16, block, (long)F * cells));
  UpdateRgbArgs a;
  a.src.frames = frames; a.src.frame_stride = frame_stride; a.src.plane = (long)h0 * w0; a.src.h0 = h0; a.src.w0 = w0;
  a.block = block;
  a.state = (int4*)plate;
  a.F = F; a.Ho = Ho; a.Wo = Wo; a.n_max = n_max;
  a.ident = h0 == Ho && w0 == Wo;
  const unsigned blocks = (unsigned)((cells + 255) / 256);
  mdqe_clear_error();
  if (is_u8) hipLaunchKernelGGL(plate_update_rgb_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(plate_update_rgb_kernel<2>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  return mdqe_launch_status();
}

extern "C" int mdqe_plate_update_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                          int F, int H, int W, int fmt, const unsigned char* block, int n_max,
                                          int* plate_y, int* plate_c, void* stream) {
  MDQE_REQUIRE(n_max >= 1 && n_max <= 256);
  MDQE_REQUIRE(F >= 0 && H > 0 && W > 0 && (fmt == 0 || fmt == 1));
  MDQE_REQUIRE((long)H * W * 4 < 0x7FFFFFFFL && (long)F * H * W < 0x7FFFFFFFL);
  const long bps = fmt ? 2 : 1;
  const int ch = (H + 1) / 2, cw = (W + 1) / 2;
  MDQE_REQUIRE(y_pitch >= W * bps && uv_pitch >= 2 * cw * bps && y_stride >= 0 && uv_stride >= 0);
  MDQE_REQUIRE(fmt == 0 || ((y_pitch | y_stride | uv_pitch | uv_stride) & 1) == 0);
  if (F == 0) return MDQE_OK;
  MDQE_REQUIRE(y != nullptr && uv != nullptr && block != nullptr && plate_y != nullptr && plate_c != nullptr);
  MDQE_REQUIRE(((uintptr_t)plate_y & 15u) == 0 && ((uintptr_t)plate_c & 15u) == 0);
  MDQE_REQUIRE(fmt == 0 || ((((uintptr_t)y | (uintptr_t)uv)) & 1u) == 0);
  const long cells = (long)H * W, ccells = (long)ch * cw;
  const long y_bytes = (F - 1) * y_stride + (H - 1) * y_pitch + W * bps, uv_bytes = (F - 1) * uv_stride + (ch - 1) * uv_pitch + 2 * cw * bps;
  const void* st[2] = {plate_y, plate_c};
  const long st_bytes[2] = {cells * 8, ccells * 16};
  for (int k = 0; k < 2; ++k)
    MDQE_REQUIRE(!meet(st[k], st_bytes[k], y, y_bytes) && !meet(st[k], st_bytes[k], uv, uv_bytes) && !meet(st[k], st_bytes[k], block, F * cells));
  MDQE_REQUIRE(!meet(plate_y, st_bytes[0], plate_c, st_bytes[1]));
  UpdateYuvArgs a;
  a.y = (const unsigned char*)y; a.y_pitch = y_pitch; a.y_stride = y_stride;
  a.uv = (const unsigned char*)uv; a.uv_pitch = uv_pitch; a.uv_stride = uv_stride;
  a.block = block;
  a.state_y = (int2*)plate_y; a.state_c = (int4*)plate_c;
  a.F = F; a.H = H; a.W = W; a.n_max = n_max;
  a.luma_blocks = (unsigned)((cells + 255) / 256);
  const unsigned blocks = a.luma_blocks + (unsigned)((ccells + 255) / 256);
  mdqe_clear_error();
  if (fmt == 0) hipLaunchKernelGGL(plate_update_yuv_kernel<0>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(plate_update_yuv_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  return mdqe_launch_status();
}

extern "C" int mdqe_plate_picture_u8(const int* plate, int Ho, int Wo, int reach, const unsigned char* fill, unsigned char* out,
                                     void* stream) {
  MDQE_REQUIRE(reach >= 0 && reach <= MAX_R);
  MDQE_REQUIRE(Ho >= 0 && Wo >= 0 && (long)Ho * Wo * 4 < 0x7FFFFFFFL);
  const long cells = (long)Ho * Wo;
  if (cells == 0) return MDQE_OK;
  MDQE_REQUIRE(plate != nullptr && fill != nullptr && out != nullptr);
  MDQE_REQUIRE(((uintptr_t)plate & 15u) == 0);
  MDQE_REQUIRE(!meet(plate, cells * 16, out, cells * 3) && !meet(plate, cells * 16, fill, 3) && !meet(out, cells * 3, fill, 3));
  PictureArgs a;
  a.p[0] = a.p[1] = plane(plate, out, 3L * Wo, Ho, Wo, reach);
  a.fill = fill;
  a.first_blocks = a.p[0].tiles_x * a.p[0].tiles_y;
  mdqe_clear_error();
  hipLaunchKernelGGL(plate_picture_kernel<0>, dim3(a.first_blocks), dim3(256), 0, (hipStream_t)stream, a, 1);
  return mdqe_launch_status();
}

extern "C" int mdqe_plate_picture_yuv420sp(const int* plate_y, const int* plate_c, int H, int W, int fmt, int reach,
                                           const unsigned short* fill_yuv, void* out_y, long out_y_pitch, void* out_uv, long out_uv_pitch,
                                           void* stream) {
  MDQE_REQUIRE(reach >= 0 && reach <= MAX_R);
  MDQE_REQUIRE(H > 0 && W > 0 && (fmt == 0 || fmt == 1) && (long)H * W * 4 < 0x7FFFFFFFL);
  const long bps = fmt ? 2 : 1;
  const int ch = (H + 1) / 2, cw = (W + 1) / 2;
  MDQE_REQUIRE(out_y_pitch >= W * bps && out_uv_pitch >= 2 * cw * bps);
  MDQE_REQUIRE(fmt == 0 || ((out_y_pitch | out_uv_pitch) & 1) == 0);
  MDQE_REQUIRE(plate_y != nullptr && plate_c != nullptr && fill_yuv != nullptr && out_y != nullptr && out_uv != nullptr);
  MDQE_REQUIRE(((uintptr_t)plate_y & 15u) == 0 && ((uintptr_t)plate_c & 15u) == 0 && ((uintptr_t)fill_yuv & 1u) == 0);
  MDQE_REQUIRE(fmt == 0 || ((((uintptr_t)out_y | (uintptr_t)out_uv)) & 1u) == 0);
  const long cells = (long)H * W, ccells = (long)ch * cw;
  const long oy_bytes = (H - 1) * out_y_pitch + W * bps, ouv_bytes = (ch - 1) * out_uv_pitch + 2 * cw * bps;
  const void* st[3] = {plate_y, plate_c, fill_yuv};
  const long st_bytes[3] = {cells * 8, ccells * 16, 6};
  for (int k = 0; k < 3; ++k)
    MDQE_REQUIRE(!meet(st[k], st_bytes[k], out_y, oy_bytes) && !meet(st[k], st_bytes[k], out_uv, ouv_bytes));
  MDQE_REQUIRE(!meet(out_y, oy_bytes, out_uv, ouv_bytes));
  MDQE_REQUIRE(!meet(plate_y, st_bytes[0], fill_yuv, 6) && !meet(plate_c, st_bytes[1], fill_yuv, 6));
  PictureArgs a;
  a.p[0] = plane(plate_y, out_y, out_y_pitch, H, W, reach);
  a.p[1] = plane(plate_c, out_uv, out_uv_pitch, ch, cw, (reach + 1) / 2);
  a.fill = fill_yuv;
  a.first_blocks = a.p[0].tiles_x * a.p[0].tiles_y;
  const unsigned blocks = a.first_blocks + a.p[1].tiles_x * a.p[1].tiles_y;
  mdqe_clear_error();
  if (fmt == 0) hipLaunchKernelGGL(plate_picture_kernel<0>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, 0);
  else hipLaunchKernelGGL(plate_picture_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, 0);
  return mdqe_launch_status();
}
