// ddz_qtrain.h -- the learner's first layer (net.py:87-94: cat, conv1..conv4, cat, max-pool) and, behind it in this file, the rest
// of the stage in front of dropout / fc1 (conv_shunzi, the views, the cat: h [n][4864] written whole), forward and backward, for a
// replay batch given as faces or as packed replay rows (QtSrc).  Included from ddz_engine.hip (inside its namespace, after
// q_feat_plane / ddz_qnet.h and face_cell / ddz_replay.h).
//
// With C = planes + 1, x[n][c][r][j] = the face planes followed by the action plane (two pointers: no cat), and the nn.Conv2d
// parameters as they lie in memory (w_k f32 [256][C][1][k], b_k f32 [256], k = 1..4: training moves them every step, so nothing
// is repacked or cached):
//   s_k = b_k[o] + sum_{c < C, j < k} w_k[o][c][0][j] * x[n][c][r][j]
//   y[n][o * 15 + r] = max_k s_k,  arg[n][o * 15 + r] = the LOWEST k - 1 that attains it (u8 0..3: max_pool2d's tie rule)
//   gw_k[o][c][0][j] = sum over (n, r) with arg == k - 1 of gy[n][o * 15 + r] * x[n][c][r][j],  gb_k[o] = the same sum of gy
// The pre-pool tensor [n][256][15][4] is never materialised.  The house pattern of k_q_feat: one thread per channel, the
// channel's 10 C weights (forward) or 10 C + 4 gradient sums (backward) in registers, the block's tile of x in LDS, read back
// as broadcasts.  A thread's fifteen values of a sample are 60 bytes from its neighbour's, so y / arg / gy go through LDS one
// sample (15,360 + 3,840 bytes, one contiguous run of global memory) at a time: a thread touches s_y[o * 15 + r] -- stride 15
// dwords, odd: conflict-free -- and the block moves the run with 16-byte accesses.
//
// Backward is deterministic without atomics, as ddz_replay.h does its scan: block b adds the tiles b, b + nb, b + 2 nb, ... in
// that order into its registers and stores them as partial b of the caller's workspace ([nb][10 C + 4][256] f32, channel
// fastest: coalesced); k_qt_reduce, one thread per gradient element, adds the nb partials in ascending b and writes the element
// at its place in the parameter's own shape.  nb = min(tiles, QT_MAX_PARTS) depends on n alone.

constexpr int QT_TILE = 8;          // samples per tile: the x tile is 19.2 KB at C = 10, y / arg of one sample 18.75 KB beside it: four blocks per CU
constexpr int QT_MAX_PARTS = 512;   // partials of the backward (two blocks per CU): 54 MB of workspace at C = 10
constexpr int QT_ROW = 15 * QH;     // 3840 = values of one sample (net.py:94's view: o * 15 + r)

constexpr int QS_OFF = QT_ROW;            // h's first conv_shunzi column (net.py:97's cat: y, then z)
constexpr int QS_LD = QT_ROW + 4 * QH;    // 4864 = the row of h [n][3840 + 256 * 4]: what fc1 consumes
constexpr int QS_WCHUNK = 32;             // channels whose 15 C weights pass through the x tile's LDS at a time (480 C floats: the tile)

struct QtW { const float* w[4]; const float* b[4]; };
struct QtG { float* w[4]; float* b[4]; };

// where x comes from.  faces (V < 0): face f32 [n][P][15] float4 + action f32 [n][15] float4.  rows (V = the face variant): sample
// i is entry e = index[i] (index null: i; clamped into [0, n_rows)) of states u8 [n_rows][176] and ids int32 [n_rows]; its planes
// are face_cell<V> of the state row, its action plane the thermometer of table[clamp(ids[e], 0, n_actions - 1)] (int8
// [n_actions][16], ddz_action_table's rows: slot j set iff count > j, as k_onehot).
struct QtSrc {
  const float4* __restrict__ face;
  const float4* __restrict__ action;
  const uint8_t* __restrict__ states;
  const int32_t* __restrict__ ids;
  const int64_t* __restrict__ index;
  const int8_t* __restrict__ table;
  int64_t n_rows;
  int n_actions;
};

inline int64_t qt_parts(int64_t n) {
  const int64_t tiles = (n + QT_TILE - 1) / QT_TILE;
  return tiles < QT_MAX_PARTS ? tiles : QT_MAX_PARTS;
}
inline int64_t qt_ws_bytes(int64_t n, int planes) { return qt_parts(n) * (10 * (planes + 1) + 4) * QH * 4; }
// the stage's backward: the first layer's partials, then conv_shunzi's [nb][15 C + 1][256]
inline int64_t qs_ws_bytes(int64_t n, int planes) { return qt_ws_bytes(n, planes) + qt_parts(n) * (15 * (planes + 1) + 1) * QH * 4; }

// the block's tile of x: faces [nt][P][15] float4 then actions [nt][15] float4 (both contiguous pieces of their tensors)
template <int P>
__device__ __forceinline__ void qt_stage_x(float4* s_x, const float4* __restrict__ face, const float4* __restrict__ action,
                                           int64_t n0, int nt) {
  for (int i = threadIdx.x; i < nt * P * 15; i += QH) s_x[i] = face[n0 * (P * 15) + i];
  for (int i = threadIdx.x; i < nt * 15; i += QH) s_x[QT_TILE * P * 15 + i] = action[n0 * 15 + i];
}
__device__ __forceinline__ int64_t qt_entry(const QtSrc& s, int64_t i) {
  int64_t e = s.index ? s.index[i] : i;
  if (e > s.n_rows - 1) e = s.n_rows - 1;
  return e < 0 ? 0 : e;
}
// the same tile from either source (same layout, and for equal inputs the same bits): the arithmetic behind it is one body
template <int P, int V>
__device__ __forceinline__ void qt_stage(float4* s_x, const QtSrc& s, int64_t n0, int nt) {
  if constexpr (V < 0) {
    qt_stage_x<P>(s_x, s.face, s.action, n0, nt);
  } else {
    static_assert(P == (V == 0 ? 4 : V == 1 ? 7 : V == 2 ? 9 : 6), "planes of the face variant");
    for (int i = threadIdx.x; i < nt * P * 15; i += QH) {
      const int ti = i / (P * 15);
      s_x[i] = face_cell<V>(s.states + qt_entry(s, n0 + ti) * STATE_ROW_BYTES, i - ti * (P * 15));
    }
    for (int i = threadIdx.x; i < nt * 15; i += QH) {
      const int ti = i / 15;
      int id = s.ids[qt_entry(s, n0 + ti)];
      id = id < 0 ? 0 : id > s.n_actions - 1 ? s.n_actions - 1 : id;
      const int c = s.table[(int64_t)id * 16 + (i - ti * 15)];
      s_x[QT_TILE * P * 15 + i] = make_float4(c > 0 ? 1.f : 0.f, c > 1 ? 1.f : 0.f, c > 2 ? 1.f : 0.f, c > 3 ? 1.f : 0.f);
    }
  }
}
template <int P>
__device__ __forceinline__ float4 qt_x(const float4* s_x, int ti, int c, int r) {
  return c < P ? s_x[(ti * P + c) * 15 + r] : s_x[QT_TILE * P * 15 + ti * 15 + r];
}

// V: the source of x (QtSrc); LD: the row stride of y in floats (QT_ROW: y alone; QS_LD: the y columns of h)
template <int P, int V = -1, int LD = QT_ROW>
__global__ __launch_bounds__(QH) void k_qt_fwd(QtSrc src, int64_t n, QtW p, float* __restrict__ y, uint8_t* __restrict__ arg) {
  constexpr int C = P + 1;
  const int o = threadIdx.x;
  __shared__ float4 s_x[QT_TILE * C * 15];
  __shared__ __attribute__((aligned(16))) float s_y[QT_ROW];
  __shared__ __attribute__((aligned(16))) uint8_t s_a[QT_ROW];
  const int64_t n0 = (int64_t)blockIdx.x * QT_TILE;
  const int nt = (int)(n - n0 < QT_TILE ? n - n0 : QT_TILE);
  qt_stage<P, V>(s_x, src, n0, nt);
  // this channel's weights, conv_k's k slots of a plane in a row (q_feat_plane's order): w_k[o][c][0][j] at (o C + c) k + j
  float w[C][10], b[4];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    int q = 0;
#pragma unroll
    for (int k = 1; k <= 4; ++k)
#pragma unroll
      for (int j = 0; j < k; ++j) w[c][q++] = p.w[k - 1][(o * C + c) * k + j];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) b[k] = p.b[k][o];
  __syncthreads();
  for (int ti = 0; ti < nt; ++ti) {
#pragma unroll 3
    for (int r = 0; r < 15; ++r) {   // (three ranks per trip: their LDS broadcasts and FMA chains interleave)
      float s0 = b[0], s1 = b[1], s2 = b[2], s3 = b[3];
#pragma unroll
      for (int c = 0; c < C; ++c) q_feat_plane(w[c], qt_x<P>(s_x, ti, c, r), s0, s1, s2, s3);
      float m = s0;
      int a = 0;
      if (s1 > m) { m = s1; a = 1; }   // strict: the lowest k keeps a tie
      if (s2 > m) { m = s2; a = 2; }
      if (s3 > m) { m = s3; a = 3; }
      s_y[o * 15 + r] = m;
      s_a[o * 15 + r] = (uint8_t)a;
    }
    __syncthreads();
    // the sample's run of y (960 float4) and of arg (240 uint4: 3840 n is a multiple of 16)
    float4* yd = (float4*)(y + (n0 + ti) * LD);
    for (int i = threadIdx.x; i < QT_ROW / 4; i += QH) yd[i] = ((const float4*)s_y)[i];
    if (arg && threadIdx.x < QT_ROW / 16) ((uint4*)(arg + (n0 + ti) * QT_ROW))[threadIdx.x] = ((const uint4*)s_a)[threadIdx.x];
    __syncthreads();
  }
}

template <int P, int V = -1, int LD = QT_ROW>
__global__ __launch_bounds__(QH) void k_qt_bwd(QtSrc src, int64_t n, const float* __restrict__ gy, const uint8_t* __restrict__ arg,
                                               float* __restrict__ part) {
  constexpr int C = P + 1;
  const int o = threadIdx.x;
  __shared__ float4 s_x[QT_TILE * C * 15];
  __shared__ __attribute__((aligned(16))) float s_g[QT_ROW];
  __shared__ __attribute__((aligned(16))) uint8_t s_a[QT_ROW];
  float gw[C][10], gb[4];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int q = 0; q < 10; ++q) gw[c][q] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) gb[k] = 0.f;
  const int64_t tiles = (n + QT_TILE - 1) / QT_TILE;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (ascending: the order of the block's sums is fixed)
    const int64_t n0 = tile * QT_TILE;
    const int nt = (int)(n - n0 < QT_TILE ? n - n0 : QT_TILE);
    qt_stage<P, V>(s_x, src, n0, nt);
    for (int ti = 0; ti < nt; ++ti) {
      const float4* gs = (const float4*)(gy + (n0 + ti) * LD);
      for (int i = threadIdx.x; i < QT_ROW / 4; i += QH) ((float4*)s_g)[i] = gs[i];
      if (threadIdx.x < QT_ROW / 16) ((uint4*)s_a)[threadIdx.x] = ((const uint4*)(arg + (n0 + ti) * QT_ROW))[threadIdx.x];
      __syncthreads();               // (covers the x tile too)
#pragma unroll 3
      for (int r = 0; r < 15; ++r) {
        const float g = s_g[o * 15 + r];
        const int a = s_a[o * 15 + r];
        // the gradient goes to the conv that won; the other three add g_k = 0 (exact: x is finite)
        const float g0 = a == 0 ? g : 0.f, g1 = a == 1 ? g : 0.f, g2 = a == 2 ? g : 0.f, g3 = a == 3 ? g : 0.f;
        gb[0] += g0; gb[1] += g1; gb[2] += g2; gb[3] += g3;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float4 x = qt_x<P>(s_x, ti, c, r);
          float(&v)[10] = gw[c];
          v[0] += g0 * x.x;
          v[1] += g1 * x.x; v[2] += g1 * x.y;
          v[3] += g2 * x.x; v[4] += g2 * x.y; v[5] += g2 * x.z;
          v[6] += g3 * x.x; v[7] += g3 * x.y; v[8] += g3 * x.z; v[9] += g3 * x.w;
        }
      }
      __syncthreads();               // (s_g / s_a, and after the last sample s_x, are free again)
    }
  }
  // partial b: [c * 10 + q][o], then the four bias sums
  float* dst = part + (int64_t)blockIdx.x * ((10 * C + 4) * QH) + o;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int q = 0; q < 10; ++q) dst[(c * 10 + q) * QH] = gw[c][q];
#pragma unroll
  for (int k = 0; k < 4; ++k) dst[(10 * C + k) * QH] = gb[k];
}

// ---- conv_shunzi (net.py:95-96: the (15,1) convolution over the same x, viewed [n][256 * 4]) ----
//   z[n][o * 4 + j] = bs[o] + sum_{c < C, r < 15} ws[o][c][r][0] * x[n][c][r][j]      written at h[n][QS_OFF + o * 4 + j]
//   gws[o][c][r][0] = sum_{n, j} gz[n][o * 4 + j] * x[n][c][r][j],   gbs[o] = sum_{n, j} gz[n][o * 4 + j]
// The house pattern again: one thread per channel, its 15 C weights (forward) or 15 C + 1 sums (backward) in registers -- they
// do not fit beside the first layer's 10 C, hence kernels of their own -- and every float4 of the x tile, read as a broadcast,
// feeds the four slots j at once.  A thread's four z of a sample are one float4, 16 bytes from its neighbour's: h / gh are
// accessed directly.  Blocks walk the tiles b, b + nb, ... (nb = qt_parts(n)) so the weights are loaded once per block.

// a channel's weights are one contiguous run of 15 C floats, 60 C bytes from the neighbour's: the block copies QS_WCHUNK channels at
// a time, coalesced, into the (not yet staged) x tile's LDS and each thread of the chunk takes its run from there
template <int C>
__device__ __forceinline__ void qs_load_w(float* s_buf, const float* __restrict__ ws, float (&w)[15 * C]) {
  static_assert(QS_WCHUNK * 15 * C <= QT_TILE * C * 15 * 4, "a chunk fits the x tile");
  const int o = threadIdx.x;
  for (int ch = 0; ch < QH / QS_WCHUNK; ++ch) {
    for (int i = threadIdx.x; i < QS_WCHUNK * 15 * C; i += QH) s_buf[i] = ws[ch * (QS_WCHUNK * 15 * C) + i];
    __syncthreads();
    if (o / QS_WCHUNK == ch) {
#pragma unroll
      for (int q = 0; q < 15 * C; ++q) {
        w[q] = s_buf[(o % QS_WCHUNK) * (15 * C) + q];
        if (q % 15 == 14) asm volatile("" ::: "memory");   // (fifteen reads in flight, not all 15 C beside the 15 C they fill)
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void qs_fma(float& acc, float a, float b) { asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(a), "v"(b)); }

template <int P, int V>
__global__ __launch_bounds__(QH) __attribute__((amdgpu_waves_per_eu(2))) void k_qs_fwd(QtSrc src, int64_t n, const float* __restrict__ ws, const float* __restrict__ bs,
                                               float* __restrict__ h) {
  constexpr int C = P + 1;
  const int o = threadIdx.x;
  __shared__ float4 s_x[QT_TILE * C * 15];
  float w[15 * C];
  qs_load_w<C>((float*)s_x, ws, w);
  const float b = bs[o];
  const int64_t tiles = (n + QT_TILE - 1) / QT_TILE;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t n0 = tile * QT_TILE;
    const int nt = (int)(n - n0 < QT_TILE ? n - n0 : QT_TILE);
    qt_stage<P, V>(s_x, src, n0, nt);
    __syncthreads();
    for (int ti = 0; ti < nt; ++ti) {
      float4 z = make_float4(b, b, b, b);
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int r = 0; r < 15; ++r) {
          const float4 x = qt_x<P>(s_x, ti, c, r);
          const float v = w[c * 15 + r];
          // (four scalar FMAs spelled out: left to itself the compiler pairs them into v_pk_fma_f32 and keeps every weight a
          // second time as a (v, v) register pair -- 30 C registers of weights, one wave per SIMD)
          qs_fma(z.x, v, x.x); qs_fma(z.y, v, x.y); qs_fma(z.z, v, x.z); qs_fma(z.w, v, x.w);
          if (r % 5 == 4) asm volatile("" ::: "memory");   // (five LDS reads in flight: not the sample's 15 C hoisted above the FMAs)
        }
      *(float4*)(h + (n0 + ti) * QS_LD + QS_OFF + o * 4) = z;
    }
    __syncthreads();                   // (s_x is free again)
  }
}

template <int P, int V>
__global__ __launch_bounds__(QH) void k_qs_bwd(QtSrc src, int64_t n, const float* __restrict__ gh, float* __restrict__ part) {
  constexpr int C = P + 1;
  const int o = threadIdx.x;
  __shared__ float4 s_x[QT_TILE * C * 15];
  float g[15 * C], gb = 0.f;
#pragma unroll
  for (int q = 0; q < 15 * C; ++q) g[q] = 0.f;
  const int64_t tiles = (n + QT_TILE - 1) / QT_TILE;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // (ascending: the order of the block's sums is fixed)
    const int64_t n0 = tile * QT_TILE;
    const int nt = (int)(n - n0 < QT_TILE ? n - n0 : QT_TILE);
    qt_stage<P, V>(s_x, src, n0, nt);
    __syncthreads();
    for (int ti = 0; ti < nt; ++ti) {
      const float4 gz = *(const float4*)(gh + (n0 + ti) * QS_LD + QS_OFF + o * 4);
      gb += (gz.x + gz.y) + (gz.z + gz.w);
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int r = 0; r < 15; ++r) {
          const float4 x = qt_x<P>(s_x, ti, c, r);
          g[c * 15 + r] += (gz.x * x.x + gz.y * x.y) + (gz.z * x.z + gz.w * x.w);
        }
    }
    __syncthreads();
  }
  // partial b: [c * 15 + r][o], then the bias sum
  float* dst = part + (int64_t)blockIdx.x * ((15 * C + 1) * QH) + o;
#pragma unroll
  for (int q = 0; q < 15 * C; ++q) dst[q * QH] = g[q];
  dst[15 * C * QH] = gb;
}

// gradient element (row e of a partial, channel o) = the sum of the nb partials in ascending order, stored at its place in the
// parameter's own shape: row e = c * 10 + q (q = k (k - 1) / 2 + j) -> gw_k[o][c][0][j]; row 10 C + k - 1 -> gb_k[o].  Blocks
// beyond 10 C + 4 (the stage's backward launches 15 C + 1 more) do the same for conv_shunzi's partials: row c * 15 + r ->
// gws[o][c][r][0], row 15 C -> gbs[o].
__global__ __launch_bounds__(QH) void k_qt_reduce(const float* __restrict__ part, int64_t nb, int C, QtG g,
                                                  const float* __restrict__ part_s, float* __restrict__ gws,
                                                  float* __restrict__ gbs) {
  const int rows = 10 * C + 4;
  const int e = blockIdx.x, o = threadIdx.x;
  if (e >= rows) {
    const int q = e - rows, rows_s = 15 * C + 1;
    const float* src = part_s + (int64_t)q * QH + o;
    float s = 0.f;
    for (int64_t b = 0; b < nb; ++b) s += src[b * rows_s * QH];
    if (q == 15 * C) gbs[o] = s;
    else gws[o * (15 * C) + q] = s;
    return;
  }
  const float* src = part + (int64_t)e * QH + o;
  float s = 0.f;
  for (int64_t b = 0; b < nb; ++b) s += src[b * rows * QH];
  // (selects, not an index: a kernel argument indexed at run time is copied to scratch)
  if (e >= 10 * C) {
    const int k = e - 10 * C;
    (k == 0 ? g.b[0] : k == 1 ? g.b[1] : k == 2 ? g.b[2] : g.b[3])[o] = s;
    return;
  }
  const int c = e / 10, q = e % 10;
  const int k = q < 1 ? 1 : q < 3 ? 2 : q < 6 ? 3 : 4;
  const int j = q - k * (k - 1) / 2;
  (k == 1 ? g.w[0] : k == 2 ? g.w[1] : k == 3 ? g.w[2] : g.w[3])[(o * C + c) * k + j] = s;
}

// The four launches of the stage for one (planes, source) instance.  first: ddz_q_first_*'s own instances (y / gy rows of 3840
// floats, no conv_shunzi); otherwise the rows of h / gh (QS_LD floats) and conv_shunzi's kernels beside the first layer's.
template <int P, int V, bool FIRST>
inline void qt_launch_fwd(const QtSrc& src, int64_t n, const QtW& p, const float* ws, const float* bs, float* h, uint8_t* arg,
                          hipStream_t st) {
  const dim3 block(QH);
  hipLaunchKernelGGL((k_qt_fwd<P, V, FIRST ? QT_ROW : QS_LD>), dim3((unsigned)((n + QT_TILE - 1) / QT_TILE)), block, 0, st, src, n, p,
                     h, arg);
  if (!FIRST) hipLaunchKernelGGL((k_qs_fwd<P, V>), dim3((unsigned)qt_parts(n)), block, 0, st, src, n, ws, bs, h);
}

template <int P, int V, bool FIRST>
inline void qt_launch_bwd(const QtSrc& src, int64_t n, const float* gh, const uint8_t* arg, const QtG& q, float* gws, float* gbs,
                          float* part, hipStream_t st) {
  const int64_t nb = qt_parts(n);
  const dim3 grid((unsigned)nb), block(QH);
  float* part_s = part + nb * (10 * (P + 1) + 4) * QH;
  hipLaunchKernelGGL((k_qt_bwd<P, V, FIRST ? QT_ROW : QS_LD>), grid, block, 0, st, src, n, gh, arg, part);
  if (!FIRST) hipLaunchKernelGGL((k_qs_bwd<P, V>), grid, block, 0, st, src, n, gh, part_s);
  hipLaunchKernelGGL(k_qt_reduce, dim3((unsigned)(10 * (P + 1) + 4 + (FIRST ? 0 : 15 * (P + 1) + 1))), block, 0, st, (const float*)part,
                     nb, P + 1, q, (const float*)part_s, gws, gbs);
}
