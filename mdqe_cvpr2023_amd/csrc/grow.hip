// The redaction margin: a label map whose GROWING labels are dilated by a bounded, exact Euclidean nearest-label rule (include/mdqe_hip.h
// has it, above mdqe_grow_labels_u8); tests/_grow_ref.py restates it in numpy and every comparison is exact.  The overlay painters take
// the grown map in place of the label map (merge.overlay_frames); no painter changes.
//
// A grown pixel needs the labels up to `radius` away, so, as in render_blur.hip, a thread block owns a TILE of 16 x 64 pixels of one
// frame plus a halo: 256 threads, phases between barriers:
//   1 stage   the (16 + 2R) x (64 + 2R) neighbourhood goes into LDS as bytes, each label already mapped to "itself if it grows, else
//             0", cells outside the picture 0 (nothing is read there).  Any non-zero cell sets the tile's LDS flag (a plain store of
//             1).  The flag therefore looks at the HALO too: a blob in a neighbouring tile grows into this one.  A tile that flags
//             nothing goes straight to the store phase and copies its labels through;
//   2 columns for the 16 tile rows by 64 + 2R columns: the minimum over |dy| <= R of the key dy^2 << 8 | label of the non-zero cells,
//             one dword per cell into a second LDS plane (NONE where the column holds none).  Keys order as (dy^2, label) does;
//   3 rows    one pixel per thread and step: a pixel whose own label grows keeps it; any other takes the minimum over |dx| <= R of
//             (dx^2 << 8) + that plane's entry, accepted where its d2 = key >> 8 is at most R^2, into a byte plane of the tile.
//             Adding dx^2 to a column's minimum keeps the order inside the column, so the two passes give the definition's
//             lexicographic minimum of (d2, label) exactly;
//   4 store   groups of 4 flat pixels laid out from the OUTPUT address: one aligned dword store per whole group, bytes for a group
//             that the tile's side cuts.  Nothing needs to be aligned.
// Lanes walk consecutive columns in both passes: byte reads of one dword broadcast and dword reads of a row are conflict-free.  The LDS
// is static, 19.6 KB whatever the radius, which leaves eight blocks on a CU: the passes wait on LDS latency and the other waves hide it.
// No data-dependent order, no atomics, no global scratch: identical from run to run.
#include "common.h"

namespace {

constexpr int TH = 16, TW = 64;                  // the tile, in pixels
constexpr int MAX_R = 32;
constexpr int PITCH = TW + 2 * MAX_R;            // cells between the rows of both LDS planes
constexpr uint32_t NONE = 0x40000000u;           // a column without a growing label: NONE + (dx^2 << 8) stays below 2^31 and is never accepted

struct GrowArgs {
  const unsigned char* labels;   // [F, H, W]
  const unsigned char* grow;     // [256]
  unsigned char* out;            // [F, H, W]
  int radius;
  int H, W;
  unsigned tiles_x, tiles_y;
  unsigned head;                 // out address mod 4: groups of 4 pixels start at flat pixels q with (q + head) % 4 == 0
  int items;                     // store items (groups of 4 pixels) per tile row
};

__device__ __forceinline__ uint32_t ld4(const unsigned char* p) {     // (any alignment)
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

__global__ __launch_bounds__(256) void grow_labels_kernel(const GrowArgs a) {
  __shared__ unsigned char s[(TH + 2 * MAX_R) * PITCH];               // the neighbourhood: the label if it grows, else 0
  __shared__ uint32_t col[TH * PITCH];                                // per tile row and staged column: min (dy^2 << 8 | label), or NONE
  __shared__ unsigned char res[TH * TW];                              // the tile's output
  __shared__ unsigned char g[256];                                    // label -> itself if it grows, else 0
  __shared__ int flag;
  const int tid = (int)threadIdx.x;
  g[tid] = tid >= 1 && a.grow[tid] != 0 ? (unsigned char)tid : (unsigned char)0;
  if (tid == 0) flag = 0;
  __syncthreads();
  unsigned b = blockIdx.x;
  const unsigned tx = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned ty = b % a.tiles_y;
  const int f = (int)(b / a.tiles_y);
  const int Y0 = (int)ty * TH, X0 = (int)tx * TW;
  const int th = a.H - Y0 < TH ? a.H - Y0 : TH, tw = a.W - X0 < TW ? a.W - X0 : TW;
  const int R = a.radius, SH = TH + 2 * R, SW = TW + 2 * R;
  const unsigned char* frame = a.labels + (long)f * a.H * a.W;
  for (int r = tid >> 7; r < SH; r += 2) {                            // (SW <= 128)
    const int c = tid & 127;
    if (c >= SW) continue;
    const int Y = Y0 - R + r, X = X0 - R + c;
    unsigned char v = 0;
    if (Y >= 0 && Y < a.H && X >= 0 && X < a.W) v = g[frame[(long)Y * a.W + X]];
    s[r * PITCH + c] = v;
    if (v != 0) flag = 1;
  }
  __syncthreads();
  const bool grown = flag != 0;                                       // (uniform over the block)
  if (grown) {
    for (int i = tid; i < th * SW; i += 256) {
      const int r = i / SW, c = i - r * SW;
      const unsigned char* q = s + (r + R) * PITCH + c;
      uint32_t best = NONE;
#pragma unroll 4
      for (int dy = -R; dy <= R; ++dy) {
        const uint32_t v = q[dy * PITCH];
        const uint32_t key = (uint32_t)(dy * dy) << 8 | v;
        best = v != 0u && key < best ? key : best;
      }
      col[r * PITCH + c] = best;
    }
    __syncthreads();
    const uint32_t r2 = (uint32_t)(R * R);
    for (int i = tid; i < th * TW; i += 256) {
      const int r = i / TW, c = i % TW;
      if (c >= tw) continue;
      const uint32_t l = frame[(long)(Y0 + r) * a.W + X0 + c];          // (asked for early: the scan below hides the load)
      uint32_t o = l;
      if (g[l] == 0) {
        const uint32_t* q = col + r * PITCH + c + R;
        uint32_t best = NONE;
#pragma unroll 4
        for (int dx = -R; dx <= R; ++dx) {
          const uint32_t key = q[dx] + ((uint32_t)(dx * dx) << 8);
          best = key < best ? key : best;
        }
        if ((best >> 8) <= r2) o = best & 0xFFu;
      }
      res[i] = (unsigned char)o;
    }
    __syncthreads();
  }
  // store: item j of tile row r is the j-th group of 4 flat pixels that meets the row's segment
  for (int it = tid; it < th * a.items; it += 256) {
    const int r = it / a.items, j = it - r * a.items;
    const long seg = ((long)f * a.H + Y0 + r) * a.W + X0;             // the segment: flat pixels [seg, seg + tw), < 2^31
    const long ps = seg - (long)((seg + a.head) & 3) + 4 * j;         // the group's first flat pixel (may lie before seg)
    const long lo = ps > seg ? ps : seg, hi = ps + 4 < seg + tw ? ps + 4 : seg + tw;
    if (lo >= hi) continue;
    const int at = r * TW + (int)(lo - seg);                          // the first of the group's results inside the segment
    if (hi - lo == 4) {
      const uint32_t v = grown ? (uint32_t)res[at] | (uint32_t)res[at + 1] << 8 | (uint32_t)res[at + 2] << 16 | (uint32_t)res[at + 3] << 24
                               : ld4(a.labels + ps);
      *(uint32_t*)(a.out + ps) = v;                                   // 4-byte aligned by the groups' layout
    } else {
      for (long q = lo; q < hi; ++q) a.out[q] = grown ? res[at + (int)(q - lo)] : a.labels[q];
    }
  }
}

}  // namespace

extern "C" int mdqe_grow_labels_u8(const unsigned char* labels, int F, int Ho, int Wo, const unsigned char* grow, int radius,
                                   unsigned char* out, void* stream) {
  MDQE_REQUIRE(radius >= 0 && radius <= MAX_R);
  MDQE_REQUIRE(F >= 0 && Ho >= 0 && Wo >= 0);
  MDQE_REQUIRE((long)Ho * Wo < 0x7FFFFFFFL && (long)F * Ho * Wo < 0x7FFFFFFFL);     // the flat pixel index of one call is 32-bit
  const long n = (long)F * Ho * Wo;
  if (n == 0) return MDQE_OK;
  MDQE_REQUIRE(labels != nullptr && grow != nullptr && out != nullptr);
  {
    // not in place: a pixel reads the labels of its neighbours, which other threads would have written
    const uintptr_t o = (uintptr_t)out, l = (uintptr_t)labels, t = (uintptr_t)grow;
    MDQE_REQUIRE(o + (uintptr_t)n <= l || l + (uintptr_t)n <= o);
    MDQE_REQUIRE(o + (uintptr_t)n <= t || t + 256u <= o);
  }
  GrowArgs a;
  a.labels = labels;
  a.grow = grow;
  a.out = out;
  a.radius = radius;
  a.H = Ho; a.W = Wo;
  a.tiles_x = (unsigned)((Wo + TW - 1) / TW);
  a.tiles_y = (unsigned)((Ho + TH - 1) / TH);
  a.head = (unsigned)((uintptr_t)out & 3u);
  // a segment of TW pixels meets at most TW / 4 + 1 groups; exactly TW / 4 where every segment starts a group (Wo is a multiple of 4
  // and so is the output address)
  a.items = TW / 4 + ((Wo & 3) == 0 && a.head == 0 ? 0 : 1);
  const long tiles = (long)F * a.tiles_y * a.tiles_x;                 // <= F * Ho * Wo < 2^31
  mdqe_clear_error();
  hipLaunchKernelGGL(grow_labels_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  return mdqe_launch_status();
}
