// moe_gate_body.inc — the body of gate_kernel and gate_modes_kernel (moe_gate.h, which says why it is
// shared as text). In scope: NB, MR, NW, U, MODE (GateMode), `a` (GateArgs) and `ex` (const
// GateModeArgs*, NULL for kGatePlain), LB (constexpr bool: the build adds a logit bias) and `lbias` (const float*,
// [E]; read only when LB), BF (constexpr bool: the operands are bf16 bit patterns behind the fp16-typed pointers,
// multiplied on v_mfma_f32_16x16x32_bf16 — the same operand and accumulator layout; nothing else differs).
  constexpr int kSlots = NW == 8 ? 4 : 3;  // partial-sum tiles in LDS at a time, per (token block, column block)
  static_assert(NW == 4 || NW == 8, "4 or 8 waves");
  static_assert(MR >= 1 && MR <= 4 && MR * kSlots * NB * 1024 <= 64 * 1024, "partial sums must fit 64 KiB of LDS");
  __shared__ gf4_t red[MR * kSlots * NB * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c16 = lane & 15, g = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * (16 * MR);
  const int E = a.E;

  // fragment rows: tokens past T and columns past E (+ 1) read a clamped, existing row; what they
  // produce is never used (masked by index below) and never stored
  const _Float16* hp[MR];
  const _Float16* wp[NB];
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    int64_t r = row0 + 16 * i + c16;
    r = r < a.T ? r : a.T - 1;
    hp[i] = a.hidden + r * a.H + 8 * g;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int c = 16 * j + c16;
    const _Float16* p = c < E ? a.w_gate + (int64_t)c * a.H : (c == E && a.w_shared) ? a.w_shared : a.w_gate;
    wp[j] = p + 8 * g;
  }

  gf4_t acc[MR][NB];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = gf4_t{0.0f, 0.0f, 0.0f, 0.0f};

  const int nsteps = a.H >> 5;
  // U consecutive K-32 steps s0 .. s0 + U - 1 of every fragment row (U * 64 contiguous bytes of each
  // row). A step past H loads step 0 instead and is skipped by mma (wave-uniform): nothing here
  // consumes a loaded register, so a prefetched group stays in flight across the previous one's MFMAs
  auto load = [&](int s0, gh8_t(&h)[U][MR], gh8_t(&w)[U][NB]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int off = s0 + u < nsteps ? (s0 + u) * 32 : 0;
#pragma unroll
      for (int i = 0; i < MR; ++i) h[u][i] = *reinterpret_cast<const gh8_t*>(hp[i] + off);
#pragma unroll
      for (int j = 0; j < NB; ++j) w[u][j] = *reinterpret_cast<const gh8_t*>(wp[j] + off);
    }
  };
  auto mma = [&](int s0, const gh8_t(&h)[U][MR], const gh8_t(&w)[U][NB]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s0 + u < nsteps) {
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j)
            if constexpr (BF)  // (in place, not through a helper: moe_gate.h, above gate_kernel)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gb8_t, w[u][j]),
                                                                  __builtin_bit_cast(gb8_t, h[u][i]), acc[i][j], 0, 0, 0);
            else
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[u][j], h[u][i], acc[i][j], 0, 0, 0);
      }
    }
  };
  {
    // wave w: groups (q NW + w) U, q = 0, 1, ...; two register buffers, the next group's loads issued
    // before the current group's MFMAs
    constexpr int kStride = NW * U;
    gh8_t hA[U][MR], wA[U][NB], hB[U][MR], wB[U][NB];
    int s = wave * U;
    if (s < nsteps) {
      load(s, hA, wA);
      for (;;) {
        const bool more1 = s + kStride < nsteps;
        if (more1) load(s + kStride, hB, wB);
        mma(s, hA, wA);
        if (!more1) break;
        const bool more2 = s + 2 * kStride < nsteps;
        if (more2) load(s + 2 * kStride, hA, wA);
        mma(s + kStride, hB, wB);
        if (!more2) break;
        s += 2 * kStride;
      }
    }
  }

  // split-K reduction, in a fixed order. 8 waves: waves 4-7 first hand everything to waves 0-3
  if constexpr (NW == 8) {
    if (wave >= 4) {
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) red[(((wave - 4) * MR + i) * NB + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] += red[((wave * MR + i) * NB + j) * 64 + lane];
    }
    __syncthreads();
  }
  // then wave w < 4 hands its partial of token block i != w to wave i (slot (w - i - 1) & 3)
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    if (i != wave && wave < 4) {
      const int slot = (wave - i - 1) & 3;
#pragma unroll
      for (int j = 0; j < NB; ++j) red[((i * 3 + slot) * NB + j) * 64 + lane] = acc[i][j];
    }
  }
  __syncthreads();
  if (wave >= MR || row0 + 16 * wave >= a.T) return;  // wave-uniform
  gf4_t x[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    x[j] = acc[0][j];
#pragma unroll
    for (int i = 1; i < MR; ++i)
      if (i == wave) x[j] = acc[i][j];
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) x[j] += red[((wave * 3 + sl) * NB + j) * 64 + lane];
    if constexpr (LB) {  // x[e] += logit_bias[e], e < E: one add, before everything that reads x (not the shared column)
      // (branch-free: a column past E reads the last bias and adds nothing)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = 16 * j + 4 * (lane >> 4) + r;
        const float b = lbias[e < E ? e : E - 1];
        x[j][r] = e < E ? x[j][r] + b : x[j][r];
      }
    }
  }

  // this lane: token t, experts 16 j + 4 g + r
  const int64_t t = row0 + 16 * wave + c16;
  const bool live = t < a.T;

  if (a.logits && live) {
    float* lrow = a.logits + t * E;
    const bool vec = (E & 3) == 0 && ((uintptr_t)a.logits & 15) == 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int e0 = 16 * j + 4 * g;
      if (vec) {
        if (e0 < E) *reinterpret_cast<gf4_t*>(lrow + e0) = x[j];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (e0 + r < E) lrow[e0 + r] = x[j][r];
      }
    }
  }

  if (a.w_shared) {  // column E: one more output column, outside the softmax and the selection
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * j + 4 * g + r == E) s = x[j][r];
    if (live && g == ((E & 15) >> 2)) a.shared_w[t] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s * -kLog2e));
  }

  uint32_t key[NB][4];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) key[j][r] = 16 * j + 4 * g + r < E ? order_key(x[j][r]) : 0u;
  if constexpr (MODE == kGateSigmoidEx) gate_sigmoid_keys<NB>(*ex, t, live, g, x, key);
  if constexpr (MODE != kGatePlain) {
    if (ex->n_group > 1) gate_group_limit<NB>(*ex, g, key);
  }

  // top-k: k rounds of (largest key, lowest index) over the lane's registers and the token's 4 lane
  // groups; choice kk is kept by lane group kk & 3 in slot kk >> 2. Sigmoid: the chosen expert's
  // score (x, which the key with its bias is not) travels with it
  uint32_t sk[4] = {0, 0, 0, 0}, mkey = 0;
  int se[4] = {0, 0, 0, 0};
  float ss[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int kk = 0; kk < a.topk; ++kk) {
    uint32_t bk = 0;
    int be = 0x7fffffff;
    float bs = 0.0f;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (key[j][r] > bk) {
          bk = key[j][r];
          be = 16 * j + 4 * g + r;
          if constexpr (MODE == kGateSigmoidEx) bs = x[j][r];
        }
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {
      const uint32_t ok = (uint32_t)__shfl_xor((int)bk, d, 64);
      const int oe = __shfl_xor(be, d, 64);
      float os = 0.0f;
      if constexpr (MODE == kGateSigmoidEx) os = __shfl_xor(bs, d, 64);
      if (ok > bk || (ok == bk && oe < be)) {
        bk = ok;
        be = oe;
        bs = os;
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * j + 4 * g + r == be) key[j][r] = 0u;
    if (kk == 0) mkey = bk;
    if ((kk & 3) == g) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q == (kk >> 2)) {
          sk[q] = bk;
          se[q] = be;
          ss[q] = bs;
        }
    }
  }

  if constexpr (MODE == kGateSigmoidEx) {
    // the chosen experts' unbiased scores, over their sum (+ 1e-20) with renormalize
    float sum = 1.0f;
    if (a.renorm) {
      sum = ((ss[0] + ss[1]) + ss[2]) + ss[3];  // (slots past topk hold 0)
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      sum += 1e-20f;
    }
    if (!live) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kk = 4 * q + g;
      if (kk < a.topk) {
        a.ids[t * a.topk + kk] = se[q];
        a.weights[t * a.topk + kk] = (a.renorm ? ss[q] / sum : ss[q]) * ex->routed_scale;
      }
    }
    return;
  }

  // softmax over the logits. (With groups: group_top is 1, so the row's maximum lies in a kept group
  // and the first choice is still the maximum)
  const float m = key_value(mkey);  // the first choice is the row's maximum
  float p[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) p[q] = 4 * q + g < a.topk ? exp_rel(key_value(sk[q]), m) : 0.0f;
  float sum = 0.0f;
  if (a.renorm) {
    sum = ((p[0] + p[1]) + p[2]) + p[3];
  } else {
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += 16 * j + 4 * g + r < E ? exp_rel(x[j][r], m) : 0.0f;
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (!live) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int kk = 4 * q + g;
    if (kk < a.topk) {
      a.ids[t * a.topk + kk] = se[q];
      if constexpr (MODE == kGatePlain) a.weights[t * a.topk + kk] = p[q] / sum;
      else a.weights[t * a.topk + kk] = p[q] / sum * ex->routed_scale;
    }
  }
