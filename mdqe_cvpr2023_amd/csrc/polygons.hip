// Track outlines: the label map's visible regions as polygons (rings of lattice corners), traced on the device.  A fourth consumer of
// the label map, beside annotate.hip, crops.hip and paths.hip.  ONE definition, integers only (include/mdqe_hip.h has the rule);
// tests/_polygon_ref.py restates it as a sequential tracer and every comparison is exact.
//
// A kernel boundary is the only hand-off between workgroups; nothing below spins, polls or syncs a grid.  The launches:
//   count   (min_area > 1 only) pixels per (label, frame): an LDS histogram per block, integer atomic adds -- counting, never indexing.
//   mark    a block owns a tile of TW x TH lattice vertices and stages the labels under it, with a one-pixel apron, in LDS (8-byte row
//           pieces).  A lane owns a vertex, looks at its 2 x 2 pixels and finds which of the four headings leave it as a CORNER (an edge
//           whose predecessor has another heading).  A wave is one SEGMENT, 64 consecutive vertices of a lattice row: ballots give every
//           vertex the number of corners before it in its segment, stored with its 4 heading bits in a 16-bit word per vertex, and the
//           segment its count.  Segments in (frame, row, column) order are the key order.
//   scan    three launches (block sums, one block over the sums, block scans): the segments' exclusive bases; the sum is the vertex total.
//   link    a lane per vertex again: each corner takes its index (segment base + word), walks its straight run along the labels to the
//           vertex where the ring turns (right before left), looks the corner there up the same way and stores itself as ITS predecessor.
//           The successor map is a bijection, so every slot is written once.  Where the total exceeds the cap nothing is stored; the
//           corners then walk their rings (stopping at the first smaller corner) and the ring starts are counted with an atomic add, so
//           that the totals are the true ones whatever the caps.
//   rank    ceil(log2(cap_vertices)) rounds of pointer jumping over the predecessor links, one launch each, double-buffered: corner i
//           holds its 2^r-th predecessor, the smallest corner index among the 2^r corners from i backwards and how many steps back that
//           one lies.  When the window covers the ring these are the ring's start and i's distance from it along the successors.
//   emit    start flags and ring sizes (packed into one 64-bit word) are scanned to ring indices and first-vertex offsets; every corner
//           writes xy[first + rank], every start corner its ring's record.
// Every kernel over the compacted corners reads the true total from device memory and leaves for indices beyond it, or altogether when
// it exceeds the cap.  Indices come from scans alone: the output order is the key order, identical from run to run.
#include "common.h"

namespace {

constexpr int TW = 64, TH = 16;                  // the mark kernel's tile, in lattice vertices: a wave per row
constexpr int LROW = 80, PIECES = 9;             // the tile's LDS row: 9 pieces of 8 bytes, pixel columns X0 - 4 .. X0 + 67
constexpr int ITEMS = 8, CHUNK = 256 * ITEMS;    // the scans: items per thread and per block
constexpr int COUNT_PIECE = 16;

struct Dims {
  int F, Ho, Wo, n;
  unsigned sx, ty;                               // segments per lattice row, tile rows per frame
};

// ---- count ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void region_count_kernel(const unsigned char* __restrict__ labels, Dims d, unsigned chunks,
                                                           int* __restrict__ cnt) {
  __shared__ int hist[256];
  const int tid = (int)threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  const int f = (int)(blockIdx.x / chunks);
  const long plane = (long)d.Ho * d.Wo;
  const long at = ((long)(blockIdx.x - (unsigned)f * chunks) * 256 + tid) * COUNT_PIECE;
  if (at < plane) {
    const unsigned char* p = labels + (long)f * plane + at;
    const int m = plane - at < COUNT_PIECE ? (int)(plane - at) : COUNT_PIECE;
    unsigned char b[COUNT_PIECE];
    if (m == COUNT_PIECE) {
      __builtin_memcpy(b, p, COUNT_PIECE);                           // (any alignment)
    } else {
#pragma unroll
      for (int q = 0; q < COUNT_PIECE; ++q) b[q] = q < m ? p[q] : p[0];
    }
    int cur = (int)b[0], run = 1;                                    // runs of equal labels: one add each
#pragma unroll
    for (int q = 1; q < COUNT_PIECE; ++q) {
      if (q >= m) break;
      if ((int)b[q] == cur) { ++run; continue; }
      atomicAdd(hist + cur, run);
      cur = (int)b[q];
      run = 1;
    }
    atomicAdd(hist + cur, run);
  }
  __syncthreads();
  const int v = hist[tid];
  if (tid >= 1 && tid <= d.n && v != 0) atomicAdd(cnt + (long)(tid - 1) * d.F + f, v);
}

// ---- mark -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mark_kernel(const unsigned char* __restrict__ labels, Dims d, int need, const int* __restrict__ cnt,
                                                   unsigned short* __restrict__ vtab, int* __restrict__ segcnt) {
  __shared__ __attribute__((aligned(8))) unsigned char tile[(TH + 1) * LROW];
  __shared__ unsigned char valid[256];
  const unsigned tx = blockIdx.x % d.sx, rest = blockIdx.x / d.sx, tyi = rest % d.ty;
  const int f = (int)(rest / d.ty), X0 = (int)tx * TW, Y0 = (int)tyi * TH, tid = (int)threadIdx.x;
  {
    bool ok = tid >= 1 && tid <= d.n;                                // a label above n, or of a region under min_area: not a region
    if (ok && need > 1) ok = cnt[(long)(tid - 1) * d.F + f] >= need;
    valid[tid] = ok ? 1 : 0;
  }
  if (tid < (TH + 1) * PIECES) {
    const int pr = tid / PIECES, pc = tid - pr * PIECES, y = Y0 - 1 + pr, x = X0 - 4 + pc * 8;
    unsigned char q[8];
    const bool row_in = y >= 0 && y < d.Ho;
    if (row_in && x >= 0 && x + 8 <= d.Wo) {
      __builtin_memcpy(q, labels + ((long)f * d.Ho + y) * d.Wo + x, 8);   // (any alignment)
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) q[k] = row_in && x + k >= 0 && x + k < d.Wo ? labels[((long)f * d.Ho + y) * d.Wo + x + k] : 0;
    }
    __builtin_memcpy(tile + pr * LROW + pc * 8, q, 8);
  }
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int row = wv; row < TH; row += 4) {                           // (wave-uniform bounds)
    const int Y = Y0 + row, X = X0 + lane;
    if (Y > d.Ho) break;
    unsigned mask = 0u;
    if (X <= d.Wo) {
      const unsigned char* up = tile + row * LROW + lane + 3;        // pixels (X-1, Y-1), (X, Y-1); a row down (X-1, Y), (X, Y)
      int a = up[0], b = up[1], c = up[LROW], e = up[LROW + 1];
      a = valid[a] ? a : 0; b = valid[b] ? b : 0; c = valid[c] ? c : 0; e = valid[e] ? e : 0;
      // heading out h is an edge of the pixel on its right; it is a corner unless an edge of that label arrives with heading h
      if (e && b != e && !(c == e && a != e)) mask |= 1u;            // E: top of (X, Y)
      if (c && e != c && !(a == c && b != c)) mask |= 2u;            // S: right of (X-1, Y)
      if (a && c != a && !(b == a && e != a)) mask |= 4u;            // W: bottom of (X-1, Y-1)
      if (b && a != b && !(e == b && c != b)) mask |= 8u;            // N: left of (X, Y-1)
    }
    int before = 0, total = 0;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const unsigned long long m = __ballot((mask >> h) & 1u);
      before += __popcll(m & below);
      total += __popcll(m);
    }
    const long line = (long)f * (d.Ho + 1) + Y;
    if (X <= d.Wo) vtab[line * (d.Wo + 1) + X] = (unsigned short)(((unsigned)before << 4) | mask);
    if (lane == 0) segcnt[line * d.sx + tx] = total;
  }
}

// ---- scans ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int shfl_up_u(int v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ unsigned long long shfl_up_u(unsigned long long v, int d) {
  const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, d, 64), hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// exclusive scan of one value per thread over the block's 256 threads; `total` is the block's sum.  Every thread calls it.
template <class U>
__device__ __forceinline__ U block_scan(U v, U* wsum, U& total) {
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  U incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const U o = shfl_up_u(incl, d);
    if (lane >= d) incl += o;
  }
  __syncthreads();                                                   // (wsum may still be read from the call before)
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  U at = incl - v;
  total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < wv) at += wsum[i];
    total += wsum[i];
  }
  return at;
}

// the length of a scan: the host's, or the device total where that is within the cap (beyond it the scan has nothing to do)
__device__ __forceinline__ long scan_length(long n_host, const int* n_dev, int cap, bool& over) {
  over = false;
  if (n_dev == nullptr) return n_host;
  const int t = *n_dev;
  over = t > cap;
  return over ? 0 : t;
}

template <class U>
__global__ __launch_bounds__(256) void scan_reduce_kernel(const U* __restrict__ in, U* __restrict__ bsum, long n_host, const int* n_dev,
                                                          int cap) {
  __shared__ U wsum[4];
  bool over;
  const long n = scan_length(n_host, n_dev, cap, over), base = (long)blockIdx.x * CHUNK;
  if (base >= n) return;                                             // (block-uniform)
  U v = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long i = base + (long)threadIdx.x * ITEMS + k;
    if (i < n) v += in[i];
  }
  U total;
  block_scan(v, wsum, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: the block sums to their exclusive bases, in place; the grand total to out_lo (its low word; out_hi: its high word),
// `zero` is cleared.  Nothing is written where the device total exceeds the cap.
template <class U>
__global__ __launch_bounds__(256) void scan_sums_kernel(U* __restrict__ bsum, long n_host, const int* n_dev, int cap, int* out_lo,
                                                        int* out_hi, int* zero) {
  __shared__ U wsum[4];
  bool over;
  const long n = scan_length(n_host, n_dev, cap, over);
  if (over) return;
  const long nb = (n + CHUNK - 1) / CHUNK;
  U carry = 0;
  for (long base = 0; base < nb; base += 256) {                      // (block-uniform)
    const long i = base + threadIdx.x;
    const U v = i < nb ? bsum[i] : (U)0;
    U total;
    const U at = block_scan(v, wsum, total);
    if (i < nb) bsum[i] = carry + at;
    carry += total;
  }
  if (threadIdx.x == 0) {
    if (out_lo != nullptr) *out_lo = (int)(unsigned)((unsigned long long)carry & 0xFFFFFFFFull);
    if (out_hi != nullptr) *out_hi = (int)(unsigned)((unsigned long long)carry >> 32);
    if (zero != nullptr) *zero = 0;
  }
}

template <class U>
__global__ __launch_bounds__(256) void scan_apply_kernel(const U* in, U* out, const U* __restrict__ bsum, long n_host, const int* n_dev,
                                                         int cap) {   // (in may be out)
  __shared__ U wsum[4];
  bool over;
  const long n = scan_length(n_host, n_dev, cap, over), base = (long)blockIdx.x * CHUNK;
  if (base >= n) return;                                             // (block-uniform)
  U x[ITEMS], v = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long i = base + (long)threadIdx.x * ITEMS + k;
    x[k] = i < n ? in[i] : (U)0;
    v += x[k];
  }
  U total;
  U at = block_scan(v, wsum, total) + bsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long i = base + (long)threadIdx.x * ITEMS + k;
    if (i < n) out[i] = at;
    at += x[k];
  }
}

// ---- link -----------------------------------------------------------------------------------------------------------------------------
struct Frame {
  const unsigned char* px;
  int Ho, Wo;
  __device__ __forceinline__ int at(int x, int y) const { return x >= 0 && x < Wo && y >= 0 && y < Ho ? (int)px[(long)y * Wo + x] : -1; }
};

// From the corner (X, Y) of label v with heading h along its straight run to the vertex where the ring turns, and the heading it
// leaves that vertex with: the right turn where label v has that edge, else the left one.
__device__ __forceinline__ void advance(const Frame& L, int v, int& X, int& Y, int& h) {
  if (h == 0) {                                                      // E: top edges of (x, Y)
    int x = X + 1;
    while (x < L.Wo && L.at(x, Y) == v && L.at(x, Y - 1) != v) ++x;
    X = x;
    h = L.at(x, Y) != v ? 1 : 3;
  } else if (h == 1) {                                               // S: right edges of (X-1, y)
    int y = Y + 1;
    while (y < L.Ho && L.at(X - 1, y) == v && L.at(X, y) != v) ++y;
    Y = y;
    h = L.at(X - 1, y) != v ? 2 : 0;
  } else if (h == 2) {                                               // W: bottom edges of (x-1, Y-1)
    int x = X - 1;
    while (x > 0 && L.at(x - 1, Y - 1) == v && L.at(x - 1, Y) != v) --x;
    X = x;
    h = L.at(x - 1, Y - 1) != v ? 3 : 1;
  } else {                                                           // N: left edges of (X, y-1)
    int y = Y - 1;
    while (y > 0 && L.at(X, y - 1) == v && L.at(X - 1, y - 1) != v) --y;
    Y = y;
    h = L.at(X, y - 1) != v ? 0 : 2;
  }
}

__device__ __forceinline__ int label_of(const Frame& L, int X, int Y, int h) {   // the pixel on the right of the edge leaving (X, Y)
  return h == 0 ? L.at(X, Y) : h == 1 ? L.at(X - 1, Y) : h == 2 ? L.at(X - 1, Y - 1) : L.at(X, Y - 1);
}

struct Corners {
  unsigned* pos;                 // X | Y << 15 | heading << 30
  int* frame;
  unsigned char* label;
  int* pred;
};

__global__ __launch_bounds__(256) void link_kernel(const unsigned char* __restrict__ labels, Dims d, long segments,
                                                   const unsigned short* __restrict__ vtab, const int* __restrict__ segbase, int* totals,
                                                   int cap, Corners co) {
  const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= segments) return;
  const int lane = (int)threadIdx.x & 63;
  const long line = s / d.sx;
  const int tx = (int)(s - line * d.sx), X = tx * TW + lane, f = (int)(line / (d.Ho + 1)), Y = (int)(line - (long)f * (d.Ho + 1));
  if (X > d.Wo) return;
  const long lines0 = (long)f * (d.Ho + 1), W1 = d.Wo + 1;
  const unsigned w = vtab[line * W1 + X];
  if ((w & 15u) == 0u) return;
  const int total = totals[0], base = segbase[s] + (int)(w >> 4);
  const Frame L{labels + (long)f * d.Ho * d.Wo, d.Ho, d.Wo};
  int rank = 0;
  for (int h = 0; h < 4; ++h) {
    if (!((w >> h) & 1u)) continue;
    const int idx = base + rank++;
    const int v = label_of(L, X, Y, h);
    int qx = X, qy = Y, qh = h;
    advance(L, v, qx, qy, qh);
    if (total <= cap) {
      const long ql = lines0 + qy;
      const unsigned w2 = vtab[ql * W1 + qx];
      const int j = segbase[ql * d.sx + qx / TW] + (int)(w2 >> 4) + __popc(w2 & ((1u << qh) - 1u));
      if (idx < total) {
        co.pos[idx] = (unsigned)X | ((unsigned)Y << 15) | ((unsigned)h << 30);
        co.frame[idx] = f;
        co.label[idx] = (unsigned char)v;
      }
      if (((w2 >> qh) & 1u) && j >= 0 && j < total) co.pred[j] = idx;
    } else {
      // too many corners to rank: count the rings, each at its smallest corner, by walking until a smaller corner (or this one) comes
      const long mine = (line * W1 + X) * 4 + h;
      for (;;) {
        const long key = ((lines0 + qy) * W1 + qx) * 4 + qh;
        if (key < mine) break;
        if (key == mine) { atomicAdd(totals + 1, 1); break; }
        advance(L, v, qx, qy, qh);
      }
    }
  }
}

// ---- rank -----------------------------------------------------------------------------------------------------------------------------
struct Jump { const int* p; const int* m; const int* o; };
struct JumpOut { int* p; int* m; int* o; };

__global__ __launch_bounds__(256) void rank_round_kernel(const int* __restrict__ totals, int cap, int round, const int* __restrict__ pred,
                                                         Jump in, JumpOut out) {
  const int total = totals[0], i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (total > cap || i >= total) return;
  const bool first = round == 0;
  int p = first ? pred[i] : in.p[i], m = first ? i : in.m[i], o = first ? 0 : in.o[i];
  if ((unsigned)p >= (unsigned)total) p = i;                         // (never, on a table the link pass wrote: a bound, not a case)
  int pp = first ? pred[p] : in.p[p];
  const int mp = first ? p : in.m[p], op = first ? 0 : in.o[p];
  if ((unsigned)pp >= (unsigned)total) pp = p;
  if (mp < m) {                                                      // (equal: the same corner, met again around the ring -- the nearer one stays)
    m = mp;
    o = (1 << round) + op;
  }
  out.p[i] = pp;
  out.m[i] = m;
  out.o[i] = o;
}

// ---- emit -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ring_flags_kernel(const int* __restrict__ totals, int cap, const int* __restrict__ pred,
                                                         const int* __restrict__ start, const int* __restrict__ dist,
                                                         unsigned long long* __restrict__ flags) {
  const int total = totals[0], i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (total > cap || i >= total) return;
  unsigned long long v = 0ull;
  if (start[i] == i) {
    int p = pred[i];
    if ((unsigned)p >= (unsigned)total) p = i;
    v = (1ull << 32) | (unsigned)(dist[p] + 1);                      // one ring, of as many corners as its last one's distance + 1
  }
  flags[i] = v;
}

__global__ __launch_bounds__(256) void emit_kernel(const int* __restrict__ totals, int cap, int cap_rings, Corners co,
                                                   const int* __restrict__ start, const int* __restrict__ dist,
                                                   const unsigned long long* __restrict__ scanned, int* __restrict__ xy,
                                                   int* __restrict__ rings) {
  const int total = totals[0], i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (total > cap || i >= total || totals[1] > cap_rings) return;
  int s = start[i];
  if ((unsigned)s >= (unsigned)total) s = i;
  const unsigned long long e = scanned[s];
  const int first = (int)(unsigned)(e & 0xFFFFFFFFull), ring = (int)(unsigned)(e >> 32), at = first + dist[i];
  const unsigned pos = co.pos[i];
  if (at >= 0 && at < total) {
    xy[2L * at] = (int)(pos & 0x7FFFu);
    xy[2L * at + 1] = (int)((pos >> 15) & 0x7FFFu);
  }
  if (s == i && ring >= 0 && ring < cap_rings) {
    int p = co.pred[i];
    if ((unsigned)p >= (unsigned)total) p = i;
    int* r = rings + 5L * ring;
    r[0] = (int)co.label[i] - 1;
    r[1] = co.frame[i];
    r[2] = first;
    r[3] = dist[p] + 1;
    r[4] = (pos >> 30) == 1u ? 1 : 0;                                // a hole's smallest corner heads S, an outer ring's E
  }
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------
struct Layout {
  long cnt, vtab, seg, ssum, pos, frame, label, pred, jp[2], jm[2], jo[2], flags, fsum, bytes;
  long vertices, segments;
  unsigned sx, ty;
};

inline Layout layout(int F, int Ho, int Wo, int cap) {
  Layout l;
  long at = 0;
  auto take = [&](long bytes) { const long here = at; at += (bytes + 15) & ~15L; return here; };
  l.sx = (unsigned)((Wo + 1 + TW - 1) / TW);
  l.ty = (unsigned)((Ho + 1 + TH - 1) / TH);
  l.vertices = (long)F * (Ho + 1) * (Wo + 1);
  l.segments = (long)F * (Ho + 1) * l.sx;
  l.cnt = take(255L * F * 4);
  l.vtab = take(l.vertices * 2);
  l.seg = take(l.segments * 4);
  l.ssum = take((l.segments / CHUNK + 2) * 4);
  l.pos = take(4L * cap);
  l.frame = take(4L * cap);
  l.label = take(cap);
  l.pred = take(4L * cap);
  for (int k = 0; k < 2; ++k) { l.jp[k] = take(4L * cap); l.jm[k] = take(4L * cap); l.jo[k] = take(4L * cap); }
  l.flags = take(8L * cap);
  l.fsum = take(((long)cap / CHUNK + 2) * 8);
  l.bytes = at;
  return l;
}

inline bool sizes_ok(int F, int Ho, int Wo, int cap_vertices) {
  return F >= 0 && Ho > 0 && Wo > 0 && Ho <= 16384 && Wo <= 16384 && (long)F * ((long)Ho * Wo) < 0x7FFFFFFFL && cap_vertices >= 1 &&
         cap_vertices <= (1 << 26);
}

}  // namespace

extern "C" long mdqe_label_polygons_workspace(int F, int Ho, int Wo, int cap_vertices) {
  if (!sizes_ok(F, Ho, Wo, cap_vertices)) return -1;
  return layout(F, Ho, Wo, cap_vertices).bytes;
}

extern "C" int mdqe_label_polygons_u8(const unsigned char* labels, int F, int Ho, int Wo, int n, int min_area, int cap_vertices,
                                      int cap_rings, int* xy, int* rings, int* totals, void* workspace, long workspace_bytes,
                                      void* stream) {
  MDQE_REQUIRE(n >= 0 && n <= 255 && min_area >= 0 && sizes_ok(F, Ho, Wo, cap_vertices) && cap_rings >= 1 && cap_rings <= (1 << 24));
  const Layout l = layout(F, Ho, Wo, cap_vertices);
  MDQE_REQUIRE(workspace_bytes >= l.bytes);
  MDQE_CHECK_PTR(totals);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0 || F == 0) {
    mdqe_clear_error();
    if (hipMemsetAsync(totals, 0, 2 * sizeof(int), st) != hipSuccess) return MDQE_ELAUNCH;
    return mdqe_launch_status();
  }
  MDQE_CHECK_PTR(labels);
  MDQE_CHECK_PTR(xy);
  MDQE_CHECK_PTR(rings);
  MDQE_CHECK_PTR(workspace);
  MDQE_REQUIRE(((uintptr_t)workspace & 15u) == 0);
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + l.cnt);
  unsigned short* vtab = (unsigned short*)(ws + l.vtab);
  int* seg = (int*)(ws + l.seg);
  int* ssum = (int*)(ws + l.ssum);
  const Corners co{(unsigned*)(ws + l.pos), (int*)(ws + l.frame), (unsigned char*)(ws + l.label), (int*)(ws + l.pred)};
  unsigned long long* flags = (unsigned long long*)(ws + l.flags);
  unsigned long long* fsum = (unsigned long long*)(ws + l.fsum);
  const Dims d{F, Ho, Wo, n, l.sx, l.ty};
  const int need = min_area > 1 ? min_area : 1, cap = cap_vertices;
  mdqe_clear_error();
  if (need > 1) {
    if (hipMemsetAsync(cnt, 0, (size_t)n * F * sizeof(int), st) != hipSuccess) return MDQE_ELAUNCH;
    const unsigned chunks = (unsigned)(((long)Ho * Wo + 256L * COUNT_PIECE - 1) / (256L * COUNT_PIECE));
    hipLaunchKernelGGL(region_count_kernel, dim3((unsigned)F * chunks), dim3(256), 0, st, labels, d, chunks, cnt);
  }
  hipLaunchKernelGGL(mark_kernel, dim3((unsigned)F * l.ty * l.sx), dim3(256), 0, st, labels, d, need, cnt, vtab, seg);
  const unsigned sblocks = (unsigned)((l.segments + CHUNK - 1) / CHUNK);
  hipLaunchKernelGGL(scan_reduce_kernel<int>, dim3(sblocks), dim3(256), 0, st, seg, ssum, l.segments, (const int*)nullptr, 0);
  hipLaunchKernelGGL(scan_sums_kernel<int>, dim3(1), dim3(256), 0, st, ssum, l.segments, (const int*)nullptr, 0, totals, (int*)nullptr,
                     totals + 1);
  hipLaunchKernelGGL(scan_apply_kernel<int>, dim3(sblocks), dim3(256), 0, st, seg, seg, ssum, l.segments, (const int*)nullptr, 0);
  hipLaunchKernelGGL(link_kernel, dim3((unsigned)((l.segments + 3) / 4)), dim3(256), 0, st, labels, d, l.segments, vtab, seg, totals, cap,
                     co);
  const unsigned cblocks = (unsigned)((cap + 255) / 256);
  int rounds = 0;
  while ((1L << rounds) < (long)cap) ++rounds;                       // ceil(log2(cap)): fixed by the cap, never read from the device
  const Jump none{nullptr, nullptr, nullptr};
  for (int r = 0; r < rounds; ++r) {
    const int to = r & 1, from = to ^ 1;
    const Jump in = r == 0 ? none : Jump{(int*)(ws + l.jp[from]), (int*)(ws + l.jm[from]), (int*)(ws + l.jo[from])};
    const JumpOut out{(int*)(ws + l.jp[to]), (int*)(ws + l.jm[to]), (int*)(ws + l.jo[to])};
    hipLaunchKernelGGL(rank_round_kernel, dim3(cblocks), dim3(256), 0, st, totals, cap, r, co.pred, in, out);
  }
  const int last = rounds > 0 ? (rounds - 1) & 1 : 0;                // (no round: a cap of 1, which no ring fits -- nothing below reads them)
  const int* start = (const int*)(ws + l.jm[last]);
  const int* dist = (const int*)(ws + l.jo[last]);
  const unsigned fblocks = (unsigned)((cap + CHUNK - 1) / CHUNK);
  hipLaunchKernelGGL(ring_flags_kernel, dim3(cblocks), dim3(256), 0, st, totals, cap, co.pred, start, dist, flags);
  hipLaunchKernelGGL(scan_reduce_kernel<unsigned long long>, dim3(fblocks), dim3(256), 0, st, flags, fsum, 0L, totals, cap);
  hipLaunchKernelGGL(scan_sums_kernel<unsigned long long>, dim3(1), dim3(256), 0, st, fsum, 0L, totals, cap, (int*)nullptr, totals + 1,
                     (int*)nullptr);
  hipLaunchKernelGGL(scan_apply_kernel<unsigned long long>, dim3(fblocks), dim3(256), 0, st, flags, flags, fsum, 0L, totals, cap);
  hipLaunchKernelGGL(emit_kernel, dim3(cblocks), dim3(256), 0, st, totals, cap, cap_rings, co, start, dist, flags, xy, rings);
  return mdqe_launch_status();
}
