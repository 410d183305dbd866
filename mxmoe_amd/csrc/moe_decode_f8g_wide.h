// moe_decode_f8g_wide.h — the decode forward for block-scaled FP8 experts at up to 64 tokens (the entries
// mxmoe_moe_decode_quant_f8g, mxmoe_moe_decode_gate_up_f8g_wide and mxmoe_moe_decode_down_f8g_wide of
// include/mxmoe_moe.h), gfx950. Included by moe_ops.hip after moe_decode_a16.h. Two kernels of their own:
//   decode_f8g_quant_kernel      one wave quantises one row with f8g_quant_row (moe_decode_f8g.h): the codes and f32
//                                group scales of MXMOE_ACT_E4M3_G128, bit for bit, to scratch tensors in global memory.
//                                Once per call and stage, where every workgroup of decode_f8g_kernel quantises all of
//                                its expert's rows itself.
//   decode_f8g_wide_kernel<DOWN> the tile: nothing is quantised here. Args, the status bits, glu_out, lp_mfma and
//                                launched are the older kernels'; the grid is tiles_shared + E * tiles workgroups of
//                                256 threads with ct = 64 or 128 columns per tile.
//
// Id scan. Up to 64 * 16 = 1024 pairs: pair q * 256 + tid in pass q, all four ballots before one barrier, then a running
// base over (pass, wave), so s_rows holds the expert's pairs in pair order.
//
// M blocks. An expert's rows go in batches of up to RB = min(64, T rounded up to 16) rows, MB = ceil(nr / 16) blocks of
// 16. Per K = 128 step the lane (r16 = lane & 15, g = lane >> 4) holds bytes [128 s + 16 g, + 16) and [+ 64, + 16) of
// weight row r16 of the wave's column group (gate_up: of the gate and of the up row) and multiplies that one fragment
// with every A block: acc[MB][NW]. The weights of an expert are therefore streamed once per batch whatever the row
// count. The fragments come from global memory straight into registers through a ring of kSteps slots: the slot of
// step s is refilled with step s + kSteps as soon as step s is multiplied, so kSteps steps stay in flight across the
// chunk barriers. More rows than RB on one expert (a token that names it twice) are further batches.
//
// A operand. The workgroup copies its expert's nr rows of codes and scales from the scratch tensors (gate_up: row
// pair / topk; down: row pair; the shared expert: row t) into LDS in chunks of KC bytes of K, two buffers: chunk c + 1
// is loaded into registers before chunk c is multiplied and written to the other buffer after it, one barrier per
// chunk. Unit u = tid + 256 i (i < 4) of a chunk is 16 bytes: row u / (KC / 16), slot u % (KC / 16); thread tid is
// scale tid % (KC / 128) of row tid / (KC / 128). f8gw_lds gives KC: the largest multiple of 128 (at most the widest
// row) whose two buffers of RB rows fit kF8gwBudget; then RB * KC / 16 <= 1024 units and RB * KC / 128 <= 256 scales.
//   [0, 32)  the head that lanes past the batch read instead of a row: zero codes and the scale 0.0f
//   buffer b codes: RB rows `row` = KC + 16 bytes apart, an odd number of 16-byte slots, so a ds_read_b128 pass over 16
//            rows is conflict-free; then scales: RB rows of KC / 128 f32, `srow` bytes apart, an odd number of dwords
// kF8gwBudget is a quarter of the CU's 160 KiB less the kernel's static LDS, so LDS admits four workgroups per CU; the
// registers (241 VGPRs in gate_up, 210 in down, no scratch) admit two.
//
// Arithmetic. No K slices: the four waves are four column groups of 16 (two passes at ct = 128). Every K group g is one
// v_mfma_scale_f32_16x16x128_f8f6f4 on a zero accumulator with unit e8m0 scales, acc_g, and
// out = fmaf(acc_g, f32_rn(sa[row][g] * sb[g][blk]), out), groups ascending across the chunks; v = fp16_rn(out): the
// GroupGEMM's contract of the type word for word. The epilogue is decode_f8g_kernel's.
#pragma once

namespace mxmoe {
namespace {
namespace decode {

constexpr int kF8gWide = 6;  // the entry pair's number beside kFirst .. kA16: no level of decode_kernel
constexpr int kWideMaxPairs = MXMOE_DECODE_WIDE_MAX_T * 16;
constexpr int kWideScan = kWideMaxPairs / kThreadsD;  // id passes
constexpr int kWideRows = 64;                         // A rows per batch at most: four M blocks
constexpr int kF8gwBudget = 160 * 1024 / 4 - kWideMaxPairs * 4 - 128;  // dynamic LDS of a workgroup

struct WideArgs {
  Args a;                  // src / src_shared: the e4m3 codes [rows][K] / [T][K_shared]
  const float* sa;         // their f32 group scales [rows][K / 128]
  const float* sa_shared;  // [T][K_shared / 128]
};

struct F8gwLds {
  int rb, kc;     // A rows per batch (a multiple of 16); bytes of K per chunk
  int row, srow;  // bytes between code rows / between scale rows of a buffer
  int scale;      // byte offset of a buffer's scales from its codes
  int buf;        // bytes of one buffer
  int bytes;      // of the whole map
};
__host__ __device__ inline F8gwLds f8gw_lds(const Args& a) {
  const int kmax = a.with_shared && a.K_shared > a.K ? a.K_shared : a.K;
  F8gwLds L;
  const int t16 = (a.T + 15) & ~15;
  L.rb = t16 < kWideRows ? t16 : kWideRows;
  L.kc = 128;
  for (int kc = 256; kc <= kmax && L.rb * kc <= 16 * 4 * kThreadsD &&  // (a thread copies four units of a chunk)
                    kF8gHead + 2 * L.rb * (kc + 16 + 4 * ((kc >> 7) | 1)) <= kF8gwBudget; kc += 128)
    L.kc = kc;
  L.row = L.kc + 16;
  L.srow = 4 * ((L.kc >> 7) | 1);
  L.scale = L.rb * L.row;
  L.buf = L.rb * (L.row + L.srow);
  L.bytes = kF8gHead + 2 * L.buf;
  return L;
}

// rows [0, rows) of src (K wide) and rows [rows, rows + rows2) of src2 (K2 wide), one wave each
struct QuantArgs {
  const uint8_t *src, *src2;
  uint8_t *codes, *codes2;
  float *scales, *scales2;
  int rows, rows2, K, K2, bf;
};
__global__ __launch_bounds__(kThreadsD) void decode_f8g_quant_kernel(QuantArgs q) {
  const int r = blockIdx.x * (kThreadsD / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r < q.rows)
    f8g_quant_row(q.src + (int64_t)r * q.K * 2, q.K, q.bf, q.codes + (int64_t)r * q.K, q.scales + (int64_t)r * (q.K >> 7));
  else if (r - q.rows < q.rows2)
    f8g_quant_row(q.src2 + (int64_t)(r - q.rows) * q.K2 * 2, q.K2, q.bf, q.codes2 + (int64_t)(r - q.rows) * q.K2,
                  q.scales2 + (int64_t)(r - q.rows) * (q.K2 >> 7));
}

// What a workgroup knows about its expert and its tile.
struct WideTile {
  const uint8_t *B, *src;  // the expert's weight codes; the A codes
  const float *SB, *ssc;   // their scales
  _Float16* out;
  const _Float16* brow;
  int K, C, tile;
  bool shared;
};

// One batch of an expert's rows: rows [r0, r0 + nr) of s_rows (the shared expert: tokens r0 + r), 16 (MB - 1) < nr <=
// 16 MB, against the tile's columns. kSteps: weight steps in flight. Every barrier is reached by all four waves: nr, the
// passes and the chunks are workgroup-uniform.
template <bool DOWN, int kSteps, int MB>
__device__ __forceinline__ void wide_batch(const Args& a, const F8gwLds& L, const WideTile& t, int r0, int nr, uint8_t* s_a,
                                           const int* s_rows) {
  constexpr int NW = DOWN ? 1 : 2;  // weight rows per lane: down 1; gate_up the gate and the up row
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = t.K, C = t.C, G = K >> 7;           // G: K groups
  const int nblk = ((DOWN ? C : 2 * C) + 127) >> 7;  // weight-row blocks: sb is [G][nblk]
  uint8_t* const s_buf = s_a + kF8gHead;
  const int spc = L.kc >> 7;     // K steps per chunk
  const int upr = L.kc >> 4;     // 16-byte units per row of a chunk
  const int passes = a.ct / 64;  // 1, or 2 for ct = 128

  // the thread's part of a chunk: four 16-byte units of codes and one scale. A unit outside the batch or past the
  // row's end loads the buffer's first bytes and is not written.
  auto src_row = [&](int r) {
    const int p = t.shared ? r0 + r : s_rows[r0 + r];  // token (shared) or pair
    return (t.shared || DOWN) ? p : p / a.topk;        // gate_up reads the pair's token
  };
  int usrc[4], udst[4], ucol[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = tid + kThreadsD * i, r = u / upr;
    ucol[i] = r < nr ? 16 * (u - r * upr) : K;  // (K: never inside a chunk)
    usrc[i] = r < nr ? src_row(r) * K + ucol[i] : 0;
    udst[i] = r * L.row + ucol[i];
  }
  const int sr = tid / spc, sj = tid - sr * spc;
  const int scol = sr < nr ? sj : G;
  const int ssrc = sr < nr ? src_row(sr) * G + sj : 0;
  const int sdst = L.scale + sr * L.srow + 4 * sj;
  lp_v4i pf[4];
  float pfs;
  auto fetch = [&](int c) {  // chunk c into registers
#pragma unroll
    for (int i = 0; i < 4; ++i)
      pf[i] = *reinterpret_cast<const lp_v4i*>(t.src + (c * L.kc + ucol[i] < K ? usrc[i] + c * L.kc : 0));
    pfs = t.ssc[c * spc + scol < G ? ssrc + c * spc : 0];
  };
  auto put = [&](int c) {  // the registers into buffer c & 1
    uint8_t* const d = s_buf + (c & 1) * L.buf;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c * L.kc + ucol[i] < K) *reinterpret_cast<lp_v4i*>(d + udst[i]) = pf[i];
    if (c * spc + scol < G) *reinterpret_cast<float*>(d + sdst) = pfs;
  };

  // the lane's A row of every M block: lanes past the batch read the head (zero codes, a zero scale) and never move
  int aoff[MB], soff[MB], orow[MB], lv[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int r = 16 * mb + r16;
    const bool live = r < nr;
    lv[mb] = live ? ~0 : 0;
    aoff[mb] = live ? kF8gHead + r * L.row + 16 * g : 0;
    soff[mb] = live ? kF8gHead + L.scale + r * L.srow : 16;
    orow[mb] = live ? (t.shared ? r0 + r : s_rows[r0 + r]) : 0;
  }

#pragma unroll 1
  for (int pass = 0; pass < passes; ++pass) {  // (workgroup-uniform; every column group lies inside C: ct | C)
    const int n = t.tile * a.ct + 16 * (wave + 4 * pass);
    // the lane's weight rows: down row n + r16; gate_up the gate and the up row of column n + r16. Their scale blocks
    // are the wave's: 16 | 128
    const uint8_t* w[NW];
    const float* ws[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      w[i] = t.B + (int64_t)(i * C + n + r16) * K + 16 * g;
      ws[i] = t.SB + ((i * C + n) >> 7);
    }
    lp_v4f acc[MB][NW];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int i = 0; i < NW; ++i) acc[mb][i] = lp_v4f{0.0f, 0.0f, 0.0f, 0.0f};

    lp_v4i lo[NW][kSteps], hi[NW][kSteps];
    float sb[NW][kSteps];
    auto loadw = [&](int u, int s) {  // step s into slot u; a step past the row: the row's first bytes, never used
      s = s < G ? s : 0;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        lo[i][u] = *reinterpret_cast<const lp_v4i*>(w[i] + s * 128);
        hi[i][u] = *reinterpret_cast<const lp_v4i*>(w[i] + s * 128 + 64);
        sb[i][u] = ws[i][s * nblk];
      }
    };
#pragma unroll
    for (int u = 0; u < kSteps; ++u) loadw(u, u);

    __syncthreads();  // the buffers of the pass or batch before are no longer read
    fetch(0);
    put(0);
    __syncthreads();
    int c = 0, cs = 0;  // the chunk in buffer c & 1 and the step inside it
    if (L.kc < K) fetch(1);

#pragma unroll 1
    for (int s0 = 0; s0 < G; s0 += kSteps) {
#pragma unroll
      for (int u = 0; u < kSteps; ++u) {
        const int s = s0 + u;
        if (s < G) {  // workgroup-uniform
          const int at = (c & 1) * L.buf;
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) {
            const uint8_t* const ap = s_a + aoff[mb] + ((at + 128 * cs) & lv[mb]);
            const lp_v4i a0 = *reinterpret_cast<const lp_v4i*>(ap);
            const lp_v4i a1 = *reinterpret_cast<const lp_v4i*>(ap + (64 & lv[mb]));
            const float sa = *reinterpret_cast<const float*>(s_a + soff[mb] + ((at + 4 * cs) & lv[mb]));
            const lp_v8i av = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
            for (int i = 0; i < NW; ++i) {
              const lp_v8i bv = {lo[i][u][0], lo[i][u][1], lo[i][u][2], lo[i][u][3],
                                 hi[i][u][0], hi[i][u][1], hi[i][u][2], hi[i][u][3]};
              const lp_v4f m = lp_mfma<true, true>(bv, 127u, av, 127u, lp_v4f{0.0f, 0.0f, 0.0f, 0.0f});
              const float sc = sa * sb[i][u];  // f32_rn(sa * sb), rounded on its own
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[mb][i][j] = fmaf(m[j], sc, acc[mb][i][j]);
            }
          }
          loadw(u, s + kSteps);
          if (++cs == spc && s + 1 < G) {  // (workgroup-uniform) the chunk is done and another follows
            ++c, cs = 0;
            put(c);
            __syncthreads();  // chunk c is staged; the other buffer is no longer read
            if ((c + 1) * L.kc < K) fetch(c + 1);
          }
        }
      }
    }

    // lane (r16, g): row 16 mb + r16 of the batch, output columns n + 4 g + 0..3
    const int col = n + 4 * g;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      if (lv[mb]) {
        typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
        h4_t o;
        if constexpr (DOWN) {
          o = h4_t{(_Float16)acc[mb][0][0], (_Float16)acc[mb][0][1], (_Float16)acc[mb][0][2], (_Float16)acc[mb][0][3]};
        } else {
          const bool has_b = t.brow != nullptr;  // workgroup-uniform
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const _Float16 bg = has_b ? t.brow[col + j] : (_Float16)0, bu = has_b ? t.brow[C + col + j] : (_Float16)0;
            const _Float16 gv = (_Float16)acc[mb][0][j], uv = (_Float16)acc[mb][NW - 1][j];
            o[j] = a.glu == kGluSwigluClamp ? glu_out<kGluSwigluClamp>(gv, uv, has_b, bg, bu, a.limit, a.c)
                                            : glu_out<kGluSilu>(gv, uv, has_b, bg, bu, a.limit, a.c);
          }
        }
        *reinterpret_cast<h4_t*>(t.out + (int64_t)orow[mb] * C + col) = o;
      }
    }
  }
}

// DOWN = false: decode_gate_up_f8g_wide; true: decode_down_f8g_wide.
template <bool DOWN, int kSteps>
__global__ __launch_bounds__(kThreadsD, 2) void decode_f8g_wide_kernel(WideArgs wa) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_a[];  // f8gw_lds's map
  __shared__ int s_rows[kWideMaxPairs];
  __shared__ int s_cnt[kWideScan * (kThreadsD / 64)];
  const Args& a = wa.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nsh = a.with_shared ? a.tiles_shared : 0;
  const int b = blockIdx.x;
  const bool shared = b < nsh;
  const int e = shared ? a.E : (b - nsh) / a.tiles;  // in [0, E] by the grid's size
  const int tile = shared ? b : (b - nsh) % a.tiles;
  const int npairs = a.T * a.topk;

  // the rows of the workgroup's expert among the call's ids, in pair order
  int nrows = a.T;
  if (!shared) {
    uint64_t m[kWideScan];
    bool bad = false;
#pragma unroll
    for (int q = 0; q < kWideScan; ++q) {
      const int p = q * kThreadsD + tid;
      const int id = p < npairs ? a.ids[p] : -1;
      m[q] = __builtin_amdgcn_ballot_w64(id == e);
      if (lane == 0) s_cnt[q * (kThreadsD / 64) + wave] = __popcll(m[q]);
      bad = bad || (p < npairs && (id < 0 || id >= a.E));
    }
    if (b == nsh && a.status) {  // one workgroup reports the ids that no workgroup matches
      if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicOr(a.status, MXMOE_DECODE_BAD_ID);
    }
    __syncthreads();
    nrows = 0;
#pragma unroll
    for (int q = 0; q < kWideScan; ++q) {
      int base = nrows;
#pragma unroll
      for (int w = 0; w < kThreadsD / 64; ++w) {
        const int c = s_cnt[q * (kThreadsD / 64) + w];
        base += w < wave ? c : 0;
        nrows += c;
      }
      if ((m[q] >> lane) & 1) s_rows[base + __popcll(m[q] & (((uint64_t)1 << lane) - 1))] = q * kThreadsD + tid;
    }
    if (nrows == 0) return;  // no token chose this expert
  }
  if (tid < kF8gHead / 4) reinterpret_cast<uint32_t*>(s_a)[tid] = 0u;
  __syncthreads();  // s_rows and the head are complete before any wave reads them (wide_batch's row maps)

  const mxmoe_moe_decode_expert ex = a.experts[e];
  if ((DOWN ? ex.kind2 : ex.kind1) != MXMOE_DECODE_W8A8_G128_E4M3) {
    if (tid == 0 && a.status) atomicOr(a.status, MXMOE_DECODE_BAD_KIND);
    return;
  }
  // the bias row of the workgroup's own expert (e < E by the grid's size): never indexed by an id
  const _Float16* brow = nullptr;
  if constexpr (!DOWN) brow = shared ? a.bias_shared : a.bias_routed ? a.bias_routed + (int64_t)e * 2 * a.C : nullptr;

  WideTile t;
  t.shared = shared, t.tile = tile, t.brow = brow;
  t.K = shared ? a.K_shared : a.K, t.C = shared ? a.C_shared : a.C;
  t.B = static_cast<const uint8_t*>(DOWN ? ex.b2 : ex.b1);
  t.SB = static_cast<const float*>(DOWN ? ex.sb2 : ex.sb1);
  t.src = static_cast<const uint8_t*>(shared ? a.src_shared : a.src);
  t.ssc = shared ? wa.sa_shared : wa.sa;
  t.out = shared ? a.out_shared : a.out;
  const F8gwLds L = f8gw_lds(a);

#pragma unroll 1
  for (int r0 = 0; r0 < nrows; r0 += L.rb) {  // (workgroup-uniform)
    const int nr = min(L.rb, nrows - r0);
    if (nr <= 16) wide_batch<DOWN, kSteps, 1>(a, L, t, r0, nr, s_a, s_rows);
    else if (nr <= 32) wide_batch<DOWN, kSteps, 2>(a, L, t, r0, nr, s_a, s_rows);
    else if (nr <= 48) wide_batch<DOWN, kSteps, 3>(a, L, t, r0, nr, s_a, s_rows);
    else wide_batch<DOWN, kSteps, 4>(a, L, t, r0, nr, s_a, s_rows);
  }
}

// ---------------------------------------------------------------------------------------------
// host side: the wide entries' own checks (before any HIP call) and the launches

inline int wide_checks(const char* fn, int64_t T, int topk, int E, int with_shared, int H, int N, int N_shared,
                       uint32_t kind_mask, int layout) {
  if (int st = f8g_checks(fn, kind_mask, layout)) return st;
  if (T < 0 || T > MXMOE_DECODE_WIDE_MAX_T || E < 1 || topk < 1 || topk > 16 || topk > E)
    return fail(MXMOE_GG_ERR_INVALID, "%s: need 0 <= T <= %d, E >= 1, 1 <= topk <= min(E, 16) (T=%lld E=%d topk=%d)", fn,
                (int)MXMOE_DECODE_WIDE_MAX_T, (long long)T, E, topk);
  if (!width_ok(H) || !width_ok(N) || (with_shared && !width_ok(N_shared)))
    return fail(MXMOE_GG_ERR_INVALID, "%s: H, N and N_shared must be multiples of 128 and <= %d (H=%d N=%d N_shared=%d)",
                fn, kMaxWidthD, H, N, N_shared);
  return MXMOE_GG_OK;
}

template <bool DOWN>
inline int launch_f8g_wide(WideArgs wa, void* stream) {
  Args& a = wa.a;
  // tiles of 128 columns while the experts that can have rows give 1024 of them (geometry()'s rule), else of 64: a
  // tile is the four waves' column groups, so it is halved no further
  const int npairs = a.T * a.topk;
  const int64_t cols = (int64_t)(a.E < npairs ? a.E : npairs) * a.C + (a.with_shared ? a.C_shared : 0);
  a.ct = cols / 128 >= 1024 ? 128 : 64;
  a.tiles = a.C / a.ct;
  a.tiles_shared = a.with_shared ? a.C_shared / a.ct : 0;
  const F8gwLds L = f8gw_lds(a);
  const dim3 grid((unsigned)((int64_t)a.tiles_shared + (int64_t)a.E * a.tiles));
  // four weight steps in flight in down; two in gate_up, whose lanes hold two weight rows (four would spill)
  hipLaunchKernelGGL((decode_f8g_wide_kernel<DOWN, DOWN ? 4 : 2>), grid, dim3(kThreadsD), L.bytes, (hipStream_t)stream, wa);
  return launched(DOWN ? "decode_down_f8g_wide_kernel" : "decode_gate_up_f8g_wide_kernel");
}

inline int launch_f8g_quant(const QuantArgs& q, void* stream) {
  const int waves = q.rows + q.rows2;
  hipLaunchKernelGGL(decode_f8g_quant_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(kThreadsD), 0, (hipStream_t)stream, q);
  return launched("decode_f8g_quant_kernel");
}

}  // namespace decode
}  // namespace
}  // namespace mxmoe
