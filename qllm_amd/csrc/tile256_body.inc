// The kernel text gemm3_kernel (gemm3.hip) and bitgemm_kernel (bitgemm.hip) share: the wave-specialised 256 x 128 x 64 tile of MW matrix
// waves and four staging waves.  Included textually into the body of both kernels, twice:
//   * with TILE256_STAGING defined, as the last statement of the unit's `if (wave >= MW) { ... }`: the staging waves' schedule.  The
//     unit has defined the two register sets `bset[2]`, `load_b(kt, set)` (request the packed words, scale and zero point of k-tile kt;
//     past the block's last tile it re-reads it) and `store_b(stage, set)` (dequantise the set into B stage `stage`);
//   * without it, behind that block: the matrix waves from their accumulators to the drain barrier, the split-K hand-off, the epilogue.
// Both halves are in ONE file because their barriers pair up: every block barrier below has its partner in the other half, and a wave
// that misses one hangs the block.
//
// Names read from the surroundings:
//   p                      the kernel's parameters: x, M, K, slabs, counters, out_bf16
//   smem, As, Bs           the dynamic LDS (tile256::kLdsBytes), the A ring [3][256][64] and the B stages [2][128 n][64 k] in it
//   tid, lane, wave        thread, lane, wave (wave-uniform: readfirstlane)
//   m0, n0                 first row / column of the block's output tile
//   KT0, KT                the block's k-tiles [KT0, KT0 + KT)
//   S, ksplit, slab_tile   split-K: blocks per output tile, this block's index among them, the tile's slab and counter index
//   PN, Pbias, Py          the layer's width, bias (or NULL) and output (grouped launches: the block's own layer)
//   MW, AM, WROWS, NP      constants: matrix waves (4 / 8), 32-row MFMA tiles per matrix wave along M (4 / 2), rows per matrix wave
//                          (128 / 64), activation DMA pieces (8 rows x 128 B) per matrix wave and k-tile (8 / 4)
//   PRIO                   constant: the matrix waves raise their issue priority over their SIMD's staging wave
//   BF                     constant: native bf16 (bf16 MFMA, one rounding of the fp32 sum to bf16)
//   N_ENDS_IN_TILE         constant: a column tile may end inside N at any multiple of 8 (bias read clamped, every 16-byte chunk of y
//                          guarded by its first column); false: at 64 or 128 columns only, which `live` below covers
//   and from tile256.hpp:  BM, BN, BK, kATile, kBTile, float16_t, bf16x8_t, lds_void_t, tile_off
#ifdef TILE256_STAGING
#undef TILE256_STAGING
    // ================================================= staging waves' schedule =========================================
    // Order of one iteration: [write B tile kt+1 from its register set] barrier [request tile kt+3 into that set].  A set is
    // requested right after the barrier that frees it and consumed two barriers later (~1.5 k-tiles of flight), and the only
    // vmcnt wait in the loop is the counted one in front of the stores (the younger set's loads stay in flight).  Nothing is
    // conditional around a load (a branch there makes hipcc's counted vmcnt collapse to vmcnt(0)): past the last tile the
    // loads re-read it and the stores fill a stage nobody reads again.
    load_b(0, bset[0]);
    load_b(1, bset[1]);
    __builtin_amdgcn_sched_barrier(0);
    store_b(0, bset[0]);
    __builtin_amdgcn_sched_barrier(0);
    load_b(2, bset[0]);
    __syncthreads();  // prologue barrier: B stage 0 holds tile 0
    for (int kt = 0; kt + 1 < KT; kt += 2) {  // two k-tiles per trip: the register sets alternate by name, no branch between them
      store_b(1, bset[1]);
      __syncthreads();  // barrier #kt
      load_b(kt + 3, bset[1]);
      __builtin_amdgcn_sched_barrier(0);
      store_b(0, bset[0]);
      __syncthreads();  // barrier #kt+1
      load_b(kt + 4, bset[0]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (KT & 1) __syncthreads();  // odd number of k-tiles: barrier #KT-1 (the tile it would publish does not exist)
    __syncthreads();  // matches the matrix waves' barrier in front of their epilogue
    if (S > 1) {          // ... and the two around the split-K ticket
      __syncthreads();
      __syncthreads();
    }
    return;
#else
  // =================================================== matrix waves ===================================================
  // Barriers, in the order of the schedule above: the prologue barrier, one per k-tile (KT of them), the drain barrier, and the two
  // around the split-K ticket where S > 1.
  const int wm = wave >> 1, wn = wave & 1;  // (MW/2) (M) x 2 (N): rows wm*WROWS.., columns wn*64..
  const int fr = lane & 31, fs = lane >> 5;  // fragment row (A: m, B: n) and k half of the 16-wide sub-step
  float16_t acc[AM][2];
#pragma unroll
  for (int a = 0; a < AM; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  half8_t fa0[AM], fb0[2], fa1[AM], fb1[2];
  auto read_frags = [&](int sa, int sb, int ks, half8_t (&fa)[AM], half8_t (&fb)[2]) {
    const half_t *Ab = As + sa * kATile, *Bb = Bs + sb * kBTile;
#pragma unroll
    for (int b = 0; b < 2; ++b) fb[b] = *(const half8_t *)(Bb + tile_off(wn * 64 + b * 32 + fr, ks * 2 + fs));
#pragma unroll
    for (int a = 0; a < AM; ++a) fa[a] = *(const half8_t *)(Ab + tile_off(wm * WROWS + a * 32 + fr, ks * 2 + fs));
  };
  // ---- activation tile by LDS-DMA: this wave owns rows wave*8 NP .. +8 NP - 1 of the 256-row tile = NP pieces of 8 rows x 128 B.
  // Piece q: lane l -> LDS row r = wave*8 NP + 8q + l/8, physical slot l%8, which holds logical 16-byte chunk (l%8) ^ lds_row_swizzle(r):
  // a piece lands lane-linear, so the swizzle is applied to the SOURCE address.  Per-lane byte offsets into x are loop constants; the
  // k-tile advance (128 B) is the scalar offset.  These waves issue no other vector memory operation and nothing is conditional around
  // a load, so the hand-placed vmcnt counts exactly the DMA pieces.
  const auto rs_x = __builtin_amdgcn_make_buffer_rsrc((void *)p.x, 0, (int)min((size_t)p.M * p.K * 2, (size_t)0x7fffffff), 0x00020000);
  int voff_x[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int r = wave * (8 * NP) + 8 * q + (lane >> 3);
    const int grow = min(m0 + r, p.M - 1);  // rows past M re-read the last row; their outputs are never stored
    voff_x[q] = grow * p.K * 2 + (((lane & 7) ^ lds_row_swizzle(r)) << 4);
  }
  // one DMA piece (8 rows x 128 B of this wave's rows) of k-tile kt into ring slot `slot`
  // (the builtin's operands are first copied into plain locals: called with template-dependent expressions, the HOST pass of
  //  hipcc silently fails to instantiate the whole kernel -- no diagnostic, just an undefined __device_stub__ at load time)
  const int rows_per_wave = 8 * NP;
  auto dma_piece = [&](int kt, int slot, int q) {
    const int so = (KT0 + min(kt, KT - 1)) * (BK * 2);
    const int vo = voff_x[q];
    lds_void_t *dst = (lds_void_t *)(As + slot * kATile + (wave * rows_per_wave + q * 8) * BK);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, dst, 16, vo, so, 0, 0);
  };
  // half of a sub-step's MFMAs: row tiles [h * AM/2, (h+1) * AM/2)
  auto mfma_half = [&](const half8_t (&fa)[AM], const half8_t (&fb)[2], int h) {
#pragma unroll
    for (int a = h * (AM / 2); a < (h + 1) * (AM / 2); ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if constexpr (BF) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, fa[a]), __builtin_bit_cast(bf16x8_t, fb[b]), acc[a][b], 0, 0, 0);
        else acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
  };

  if constexpr (PRIO) __builtin_amdgcn_s_setprio(2);  // the matrix wave outranks its SIMD's staging wave for issue slots
#pragma unroll
  for (int q = 0; q < NP; ++q) dma_piece(0, 0, q);
#pragma unroll
  for (int q = 0; q < NP; ++q) dma_piece(1, 1, q);
  if constexpr (NP == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // tile 0's pieces have landed (tile 1's still in flight)
  else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();                      // prologue barrier (the staging waves' __syncthreads)
#pragma unroll
  for (int q = 0; q < NP / 4; ++q) dma_piece(2, 2, q);
  read_frags(0, 0, 0, fa0, fb0);
  // The issue order is pinned (sched_barrier): left alone, hipcc sinks every fragment read to just above its first use
  // (fewest live registers) and the lone matrix wave of the SIMD then sits out each LDS round trip with an idle matrix pipe.
  // A DMA piece costs 60-180 issue cycles (MI355X_MICROARCH.md): one goes behind every four MFMAs (128 cycles of matrix-pipe
  // work), never eight in a row (first version: all eight right after the barrier -- the pipe ran dry behind them).
  // Between barrier #kt-1 and barrier #kt the wave requests the NP pieces of tile kt+2 (slot (kt+2)%3, freed by barrier
  // #kt-1): the first NP/4 beside sub-step 3 of tile kt-1, the rest beside sub-steps 0..2 of tile kt.  At barrier #kt the
  // pieces of tile kt+1 are older than those NP: vmcnt(NP) retires exactly them.
#define T256_SB() __builtin_amdgcn_sched_barrier(0)
  // NP == 4 (one piece per sub-step): the piece goes BETWEEN the two halves of the sub-step's MFMAs, not behind them (round 4,
  // profiles/logs/r04p_time_native.log: +1-2 % on all three shapes; alternating the position between the two matrix waves of a SIMD: none)
#define T256_PIECE_MID(kt_, slot_, q8, q4) { dma_piece(kt_, slot_, NP == 8 ? q8 : q4); T256_SB(); }
#define T256_PIECE_END(kt_, slot_, q8, q4) if constexpr (NP == 8) { dma_piece(kt_, slot_, q8); } T256_SB();
  int sa = 0;  // A ring slot of tile kt (kt % 3)
  for (int kt = 0; kt < KT; ++kt) {
    const int sb = kt & 1;
    const int sa1 = (sa == 2) ? 0 : sa + 1, sa2 = (sa == 0) ? 2 : sa - 1;  // slots of tiles kt+1, kt+2
    // pieces per sub-step: NP / 4 (2 or 1), one behind each half (NP = 8) or behind the first half (NP = 4) of its MFMAs;
    // piece indices: sub-step 3 of the previous tile took [0, NP/4), sub-steps 0..2 take the rest
    read_frags(sa, sb, 1, fa1, fb1);
    T256_SB();
    mfma_half(fa0, fb0, 0); T256_SB();
    T256_PIECE_MID(kt + 2, sa2, 2, 1)
    mfma_half(fa0, fb0, 1); T256_SB();
    T256_PIECE_END(kt + 2, sa2, 3, 1)  // sub-step 0
    read_frags(sa, sb, 2, fa0, fb0);
    T256_SB();
    mfma_half(fa1, fb1, 0); T256_SB();
    T256_PIECE_MID(kt + 2, sa2, 4, 2)
    mfma_half(fa1, fb1, 1); T256_SB();
    T256_PIECE_END(kt + 2, sa2, 5, 2)  // sub-step 1
    read_frags(sa, sb, 3, fa1, fb1);
    T256_SB();
    mfma_half(fa0, fb0, 0); T256_SB();
    T256_PIECE_MID(kt + 2, sa2, 6, 3)
    mfma_half(fa0, fb0, 1); T256_SB();
    T256_PIECE_END(kt + 2, sa2, 7, 3)  // sub-step 2
    // barrier #kt: my fragment reads of tile kt are complete (lgkmcnt(0)) and my DMA pieces of tile kt+1 have landed
    // (vmcnt(NP): only tile kt+2's are still in flight).  After it: B stage sb and A slot sa are free, tile kt+1 is complete.
    // (The raw s_barrier with explicit counts: __syncthreads() would drain the DMA ring with vmcnt(0).)
    if constexpr (NP == 8) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    T256_SB();
    read_frags(sa1, sb ^ 1, 0, fa0, fb0);  // past the last tile: stages nobody uses
    T256_SB();
    mfma_half(fa1, fb1, 0); T256_SB();
    T256_PIECE_MID(kt + 3, sa, 0, 0)
    mfma_half(fa1, fb1, 1); T256_SB();
    T256_PIECE_END(kt + 3, sa, 1, 0)  // sub-step 3
    sa = sa1;
  }
  // (a last column tile that ends inside its 128 columns: the matrix waves whose 64 columns are all past N run this loop too -- their
  //  DMA pieces feed the other waves' rows, their MFMAs on B columns nobody stores cost no time -- and leave before the epilogue)
  const bool live = n0 + wn * 64 < PN;
#undef T256_PIECE_MID
#undef T256_PIECE_END
#undef T256_SB
  __builtin_amdgcn_s_setprio(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // stray DMA pieces past the last tile: land before the LDS is reused
  __builtin_amdgcn_s_barrier();                                // drain barrier (matched by the staging waves' final barrier)

  // ---- split-K: publish the fp32 partial tile; the last block to arrive sums the S partials in fixed order (deterministic).
  // Write-through (sc1) stores, every storing wave drains them, one relaxed agent-scope ticket per block, the last arriver reads
  // with sc1 loads and re-arms the counter.  Slab element (tile, split, wave, register, lane): 256 contiguous bytes per instruction.
  if (S > 1) {
    int &s_ticket = *(int *)(smem + 24 * 1024);  // past the epilogue's wave-private regions (8 x 4.5 KB)
    constexpr int WREGS = AM * 2 * 16;
    float *slab = p.slabs + ((size_t)slab_tile * S + ksplit) * (size_t)(BM * BN) + (size_t)wave * (WREGS * 64) + lane;
#pragma unroll
    for (int a = 0; a < AM; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) st_sc1(slab + ((a * 2 + b) * 16 + r) * 64, acc[a][b][r]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(p.counters + slab_tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != S - 1) return;
#pragma unroll
    for (int a = 0; a < AM; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    for (int sp = 0; sp < S; ++sp) {
      const float *src = p.slabs + ((size_t)slab_tile * S + sp) * (size_t)(BM * BN) + (size_t)wave * (WREGS * 64) + lane;
#pragma unroll
      for (int a = 0; a < AM; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][b][r] += ld_sc1(src + ((a * 2 + b) * 16 + r) * 64);
    }
    if (tid == 0) __hip_atomic_store(p.counters + slab_tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!live) return;  // (columns past N: no bias, no store; the block's last barrier is behind it)

  // ---- epilogue: + bias, round once, transpose through wave-private LDS, 16-byte row-contiguous stores ---------------------
  // C/D layout of 32x32 tiles: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  (All fragment reads that
  // matter completed before the last barrier; the stray ones above only fill registers.)
  half_t *ep = smem + wave * (32 * 72);  // 32 rows x 64 cols, row stride 72 halves (144 B)
  float bv[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int n = n0 + wn * 64 + b * 32 + fr;
    if constexpr (N_ENDS_IN_TILE) bv[b] = Pbias ? (float)Pbias[min(n, PN - 1)] : 0.f;
    else bv[b] = Pbias ? (float)Pbias[n] : 0.f;
  }
#pragma unroll
  for (int a = 0; a < AM; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fs;
        const float v = acc[a][b][r] + bv[b];
        // bf16 y from fp16 x (the caller's pre-pass converted x): the result is rounded to fp16 and then to bf16, as the
        // reference's shim does (fp16 kernel output .to(bfloat16), quant_linear_awq.py:29-36, 144-146)
        if constexpr (BF) ((uint16_t *)ep)[row * 72 + b * 32 + fr] = f32_to_bf16(v);  // (native bf16: one rounding of the fp32 sum)
        else if (p.out_bf16) ((uint16_t *)ep)[row * 72 + b * 32 + fr] = f32_to_bf16((float)(half_t)v);
        else ep[row * 72 + b * 32 + fr] = (half_t)v;
      }
    // 32 rows x 128 B = 256 chunks of 16 B: 4 per lane (wave-private region: no barrier, the wave's own LDS ops are ordered)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int c = lane + 64 * h, row = c >> 3, ch = c & 7;
      const uint4_t v = *(const uint4_t *)(ep + row * 72 + ch * 8);
      const int m = m0 + wm * WROWS + a * 32 + row;
      // (the column is summed as int on one side and into the 64-bit offset on the other: either spelling, used for both, changes the
      //  other unit's vector code)
      if constexpr (N_ENDS_IN_TILE) {
        const int n = n0 + wn * 64 + ch * 8;  // (PN % 8 == 0: a chunk is inside N or outside it)
        if (m < p.M && n < PN) *(uint4_t *)((half_t *)Py + (size_t)m * PN + n) = v;
      } else {
        if (m < p.M) *(uint4_t *)((half_t *)Py + (size_t)m * PN + n0 + wn * 64 + ch * 8) = v;
      }
    }
  }
#endif
