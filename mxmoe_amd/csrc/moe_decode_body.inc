// moe_decode_body.inc — the statements with which the three decode kernels of moe_decode.h begin (decode_kernel<DOWN>,
// decode_ex_kernel<DOWN>, decode_wo_kernel<DOWN>; `a`: the kernel's Args, ArgsEx or ArgsWo): the workgroup's expert and column tile, the rows of that
// expert among the call's ids (in pair order, into s_rows), the report of ids that no workgroup matches, and the
// expert's record and kind. Leaves s_a, s_rows, s_scale, shared, e, tile, nrows, ex and kind to the kernel; a
// workgroup without rows, or with a kind outside the call's mask, returns here. Included as text, not called: the
// first two entries' kernels are compiled from these statements as they were when the kernel held them itself.
  extern __shared__ __attribute__((aligned(16))) uint8_t s_a[];  // [rb][lds_row]
  __shared__ int s_rows[kMaxPairs];
  __shared__ int s_cnt[kThreadsD / 64];
  __shared__ _Float16 s_scale[kBatchRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nsh = a.with_shared ? a.tiles_shared : 0;
  const int b = blockIdx.x;
  const bool shared = b < nsh;
  const int e = shared ? a.E : (b - nsh) / a.tiles;  // in [0, E] by the grid's size
  const int tile = shared ? b : (b - nsh) % a.tiles;
  const int npairs = a.T * a.topk;

  int nrows = a.T;
  if (!shared) {
    const int id = tid < npairs ? a.ids[tid] : -1;
    const bool hit = id == e;
    const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    if (b == nsh && a.status) {  // one workgroup reports the ids that no workgroup matches
      const bool bad = tid < npairs && (id < 0 || id >= a.E);
      if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicOr(a.status, MXMOE_DECODE_BAD_ID);
    }
    __syncthreads();
    int base = 0;
    nrows = 0;
#pragma unroll
    for (int w = 0; w < kThreadsD / 64; ++w) {
      base += w < wave ? s_cnt[w] : 0;
      nrows += s_cnt[w];
    }
    if (nrows == 0) return;  // no token chose this expert
    if (hit) s_rows[base + __popcll(m & (((uint64_t)1 << lane) - 1))] = tid;
  }

  const mxmoe_moe_decode_expert ex = a.experts[e];
  const int kind = DOWN ? ex.kind2 : ex.kind1;
  if (kind < 0 || kind > 31 || !((a.kind_mask >> kind) & 1u)) {  // (the mask holds existing kinds only: the entry's check)
    if (tid == 0 && a.status) atomicOr(a.status, MXMOE_DECODE_BAD_KIND);
    return;
  }
