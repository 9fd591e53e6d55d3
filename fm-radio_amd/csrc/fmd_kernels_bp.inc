// =============================================================================================
// k_extract_bp — FMD_FLAG_FAST_MATH, round 5: the extract stage with the harmonic mixers BEHIND the decimating FIRs.
//
// The reference mixes every 128 kHz sample of the analytic signal a[t] = fm_out[t - 32] + j hilbert(fm_out)[t] with the pilot NCO's
// 2nd / 3rd harmonic and then low-passes and decimates (broadcast_fm_demod.cpp:463-536, apply_harmonic_pll.cpp:88-139):
//     y[m] = sum_tau h[tau] a[t0 + tau] e^{j 2 pi (H dt[t0 + tau] + off)},        t0 = M (m + 1) - 128
// The NCO phase is dt[t] = p(t) - 19 (t + 1) / 128 (turns): an exactly periodic carrier and the loop's deviation p(t), the span cubics
// of k_pll_sparse — a line a few Hz wide, i.e. over the FIR's 128 taps (1 ms) p(t_c) + p'(t_c) (t - t_c) to second order.  Then
//     y[m] = e^{j 2 pi (H p(t_c) + off - H 19 (t0 + 1) / 128)} (S0[m] + j 2 pi H p'(t_c) S1[m]),    S_i[m] = sum_u G_i[u] fm_out[M m - 188 + (M - 4) + u]
// where G0 = (h[.] e^{-j 2 pi H 19 . / 128}) * (delta_32 + j hilbert) is ONE fixed complex band-pass FIR of 192 taps on the REAL signal
// fm_out, and G1 the same with the taps (tau - 63.5) h[tau]: the Hilbert FIR, both mixers at 128 kHz and their bf16 splits (two thirds of
// round 4's k_extract_mfma's VALU instructions: DESIGN_HISTORY.md section 8) become more rows of matrix-core work, and what is left per OUTPUT is one rotation.  Without the
// first-order term the filter is seen shifted by H p' Hz — tools/proto/bandpass_extract.py against the oracle: L-R 4e-6 per Hz of NCO
// offset (taken: 7e-6 RMS during acquisition, < 1e-6 in lock, bar 1e-4); the RDS rails 1e-3 of their RMS per Hz (their filter's
// transition band is where the RDS spectrum lives): they carry the S1 term (hi x hi product only: it is a correction of 1e-3) and are
// then within 1e-5 of their RMS from the first block on.
//
// Workgroup = station x 4 NT tiles of 256 audio samples, A WAVEFRONT OWNS A TILE (wavefront w: tiles tile_first + w, + 4, ...).  Window
// W[i] = fm_out[4 i0 - 188 + i], i < 1212, staged as bf16 hi / lo halves in the wavefront's own 6 KB of LDS.  Every FIR family is laid out on
// ONE geometry — column c of a 16-column tile reads W[64 c + t], t < 256: 8 K-steps —
//   family 0: L+R        rows = 16 outputs,       Y[m][c] = lpr[16 c + m],       A[m][t] = h_lpr[t - 32 - 4 m]
//   1, 2:     L-R re, im rows = 16 outputs,       Y[m][c] = S0_rail[16 c + m],   A[m][t] = G0_rail[t - 4 m]
//   3:        RDS S0     rows = 8 outputs x rail, Y[2 o + r][c] = S0_r[8 c + o], A[2 o + r][t] = G0_r[t - 4 - 8 o]
//   S1:       RDS first-order term, rows as RDS S0 (hi x hi only)
// so that ONE pair of window operands per K-step serves all four families and S1 (13 matrix instructions on 11 LDS reads; the three bf16
// products of a family go into one accumulator, four matrix instructions apart), and with the window's padding of 8 elements per 32 every
// operand read is a 16-byte aligned ds_read_b128 on a column stride of 160 bytes = 10 sixteen-byte slots: under the instruction's real
// lane groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... MI355X_MICROARCH.md) that is conflict-free, as 2, 6 and 14 slots (mod 16) would
// be and no odd stride is.  (Padding of 4 per 32 — 144 bytes, every second read only 8-byte aligned, i.e. ds_read2_b64 at half the rate on
// 32 banks — measured SQ_LDS_BANK_CONFLICT at 52 % of the kernel's LDS cycles.)
// The TAP operands (v_mfma_f32_16x16x32_bf16's A: lane l = row l % 16, k = 8 (l / 16) .. + 7) come from zero-padded tap tables in LDS,
// staged once per workgroup (16 KB from L2) and read per K-step.
// The outputs come straight from the accumulators: lane (column c, k) holds rows 4 k .. 4 k + 3 — audio outputs 16 c + 4 k .. + 3 (one
// span cubic, two 16-byte stores), RDS outputs 8 c + 2 k, + 1 (one 16-byte store), at most one of the block's every-10th phase
// estimates: the rotation, MixAudio, the estimate's arctangent once per lane.  No result arrays, no barrier in the tile loop; what a
// workgroup shares is the tap tables, the block's L-R offset and S_old.  Forms measured on the way (profiles/round5/extract_ab.txt; ms in
// the step of a 4096-station block): a family per wavefront with operand images through L1 0.29, tap tables read as ds_read2_b64 0.187,
// images in 72 registers at three workgroups per CU 0.112-0.117, conflict-free tables at five 0.104; a wavefront per tile 0.086-0.089.
// Block edge: the reference mixes a block's samples with that block's L-R offset, so the first 31 outputs of a block carry both the old
// and the new offset: y = e^{j ...}(e^{j off_cur}(S - S_old) + e^{j off_prev} S_old), S_old[m] = the taps tau < 124 - 4 m (those that reach
// into the previous block).  S_old is linear in the window's first 188 samples: a fixed 62 x 188 matrix per cut-off (Buffers::bp_edge,
// made on the host from the composite of the TRUNCATED taps, stored as fp16), applied with fp32 accumulation in the prologue of the
// workgroup that holds the block's first tile, 8 lanes per output — its rows are asked for with the kernel's first loads.  (First form:
// Hilbert FIR and carrier of the previous block's 124 analytic samples, a barrier, 31 truncated FIRs, a barrier: 0.014 ms of the kernel's
// 0.131.  As a 62 x 192 product on the matrix cores by the wavefront that owns the tile: slower — its 48 operand loads wait for L2 in turn.)
// =============================================================================================
struct ExtractGeomB {
    static constexpr int TA = 256, WN = 4 * TA + 188, WNP = 1216;
    static constexpr int NBW = (WNP + 8 * (WNP >> 5)) / 2;               // words per bf16 half-array (8 elements of padding after every 32)
    static constexpr int KS = 8;                                         // K-steps of every family: a column's window is W[64 c .. 64 c + 255]
    static constexpr int EDGE = 124;                                     // analytic samples of the previous block the first outputs reach back to
    __device__ static __forceinline__ int pad(int i) { return i + 8 * (i >> 5); }
    static_assert(WNP % 32 == 0 && WNP >= 64 * 15 + 32 * KS, "reach of the operands");
    static_assert(WN % 4 == 0 && WN / 4 - 256 <= 64 && WNP / 4 - 256 <= 64, "four quads per lane and one more for lanes 0 .. 47 stage the window");
};
// Tap tables: a lane's operand of K-step s is 8 CONSECUTIVE taps, g[32 s + 8 k - shift - stride o .. + 7], read from zero-padded TAP TABLES in LDS
// (bf16, kBpTL elements each, tap i at element kBpPadL + i).  A family's block is four tables,
// [hi, copy 0][hi, copy 4][lo, copy 0][lo, copy 4]: copy 4 is the table moved on by four elements, read by the odd rows (their band offset
// 4 o is 4 mod 8) so that EVERY operand read is a 16-byte aligned ds_read_b128; the RDS families' rows (o, rail) read [re hi][im hi][re lo][im lo],
// each stored moved on by four (their offset 4 + 8 o).  A table is 896 bytes = 128 (mod 256): the two tables one read instruction touches lie
// 8 sixteen-byte slots apart, and with the Toeplitz band (neighbouring rows read overlapping addresses: broadcast) the instruction's lane
// groups hit 14 different slots — conflict-free (DESIGN.md section 3).  Buffers::bp_tab per cut-off slot: L+R, L-R re, L-R im blocks;
// Buffers::rds_bp_tab: RDS S0 block, then S1 [re hi][im hi].
static constexpr int kBpTabU4 = kBpTL * 2 / 16, kBpTabSlotU4 = kBpSlotTabs * kBpTabU4;     // (kBpPadL, kBpTL, the table counts: fmd_tables.h)
static_assert(kBpTL * 2 % 256 == 128 && kBpTL >= kBpPadL + 4 + 32 * ExtractGeomB::KS + 8 && kBpPadL >= 32 + 4 * 14 + 8 && kBpPadL % 8 == 0, "tap table geometry");

// sum over groups of 8 adjacent lanes (every lane of a group gets it)
__device__ __forceinline__ float oct_sum_f32(float v) {
    {   // + v[i ^ 4]: row_shl:4 into lanes 0-3 and 8-11 of a row, row_shr:4 into the others
        const int up = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x104, 0xf, 0x5, true);
        v += __int_as_float(__builtin_amdgcn_update_dpp(up, __float_as_int(v), 0x114, 0xf, 0xA, false));
    }
    v += dpp0<0x4E>(v);
    v += dpp0<0xB1>(v);
    return v;
}

// SPW = stations per workgroup (round 6).  2: one workgroup stages the tap tables and fetches the block edge's matrix ONCE for two stations
// (every workgroup of a 64 ms block is a station's first AND only one: 16 KB of tables and 24 KB of matrix rows from L2 against 39 KB of window
// data) — for batches that still give the chip 1536 workgroups and whose stations share their cut-offs (fmd_plan.cpp make_block_plan).  Same arithmetic per
// output: results are bit-identical to SPW = 1.
template <int SPW>
__global__ __launch_bounds__(256, 4) void k_extract_bp(Dims d, int nt, const float* __restrict__ fo_pl, const float4* __restrict__ pll_poly,
                                                        const uint4* __restrict__ bp_tab, const int2* __restrict__ aud_idx, const uint4* __restrict__ rds_tab,
                                                        const uint4* __restrict__ bp_edge, const float* __restrict__ mixctl, float* __restrict__ state,
                                                        float* __restrict__ audio, float2* __restrict__ rds, float* __restrict__ lmr_est,
                                                        float* __restrict__ lpr_out, float* __restrict__ lmr_out, int keep_taps,
                                                        const float* __restrict__ lmr_est_prev, int field_cur, int field_prev, float* __restrict__ rds_pow) {
    using G = ExtractGeomB;
    constexpr int TA = G::TA;
    __shared__ __attribute__((aligned(256))) uint16_t tabs[(kBpSlotTabs + kBpRdsTabs) * kBpTL];               // the station's tap tables: [family 0 .. 3][4 tables], then S1's two
    __shared__ __attribute__((aligned(16))) uint32_t win[4][2 * G::NBW];              // per wavefront: its tile's window as bf16 halves, two per word, [hi | lo]
    __shared__ float2 s_old[SPW][SPW == 1 ? 32 : 31];
    __shared__ float off_s[SPW];
    float* wf32 = reinterpret_cast<float*>(win[3]);      // block's first tile, AHEAD of the tile loops: the window's first 192 samples in fp32
    static_assert(sizeof(tabs) + sizeof(win) + sizeof(s_old) + sizeof(off_s) <= 40960, "four workgroups per CU");

    const bool no_edge = (nt & 0x10000) != 0;    // (development builds only: timing without the first tile's extra phase)
    nt &= 0xffff;
    const int tiles = d.n_audio / TA, per_wg = 4 * nt, groups = (tiles + per_wg - 1) / per_wg;
    // SPW == 2: groups == 1 (the host's choice), the workgroup's wavefronts walk the 2 x tiles tiles of stations c, c + 1 in turn
    const int c = SPW * (blockIdx.x / groups), tile_first = (blockIdx.x % groups) * per_wg;
    const bool two = SPW == 2 && c + 1 < d.C;
    const int tid = threadIdx.x;
    __builtin_assume(tid >= 0 && tid < 256);
    const int lane = tid & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = d.n_fm_out;
    const float* fo_c0 = fo_pl + (size_t)c * (kFoPad + n) + kFoPad;
    const float4* po_c0 = pll_poly + (size_t)c * (1 + n / kSpan) + 1;
    const float off_prev0 = st(state, field_prev, d.C, c), off_prev1 = two ? st(state, field_prev, d.C, c + 1) : 0.0f;
    float off_cur0 = lmr_est_prev ? 0.0f : st(state, field_cur, d.C, c), off_cur1 = (lmr_est_prev || !two) ? 0.0f : st(state, field_cur, d.C, c + 1);
    const bool edge = tile_first == 0 && !no_edge;
#ifdef FMD_X_PROBE
    // development probe (tools/dbg/bp_probe.py): cycles of wavefronts 0 and 3 of every 61st workgroup per phase, summed over their tiles
    const bool xp_on = (blockIdx.x % 61) == 0;
    unsigned long long xp_t = __builtin_readcyclecounter();
    const unsigned long long xp_c0 = xp_t, xp_w0 = wall_clock64();
    if (xp_on && threadIdx.x == 0) atomicAdd(&g_x_probe[7], (unsigned long long)nt);
#endif

    // ---- workgroup prologue: last block's phase estimates, the station's tap tables, (block's first tile) S_old's matrix and samples
    float ev[kLmrInlineMax / kWave];
    const bool est_wave = wv == 0 || (wv == 1 && two);      // wavefront 0: station c's estimates, wavefront 1: station c + 1's
    if (lmr_est_prev && est_wave) {
#pragma unroll
        for (int k = 0; k < kLmrInlineMax / kWave; k++) ev[k] = (lane + kWave * k < d.n_est) ? lmr_est_prev[(size_t)(c + wv) * d.n_est + lane + kWave * k] : 0.0f;
    }
    uint4 em[kBpEdgeU4];                         // the block's first tile: this thread's 24 columns x (re, im) of S_old's matrix (fp16), row tid / 8
    float4 qe, qe1;
    {
        const int2 slot = aud_idx[c];
        if (edge) {
            if (tid < 48) qe = *reinterpret_cast<const float4*>(fo_c0 - 188 + 4 * tid);
            if (SPW == 2 && two && tid < 48) qe1 = *reinterpret_cast<const float4*>(fo_c0 + (kFoPad + n) - 188 + 4 * tid);
            if (tid < kBpEdgeRows) {
                const uint4* ep = bp_edge + ((size_t)slot.y * kBpEdgeRows + tid) * kBpEdgeU4;
#pragma unroll
                for (int k = 0; k < kBpEdgeU4; k++) em[k] = ep[k];
            }
        }
        constexpr int NU4 = (kBpSlotTabs + kBpRdsTabs) * kBpTabU4;
#pragma unroll
        for (int r = 0; r < (NU4 + 255) / 256; r++) {
            const int j = tid + 256 * r;
            if (j < NU4) {
                const int blk = j / (4 * kBpTabU4), within = j % (4 * kBpTabU4);        // block 0: L+R, 1: L-R re, 2: L-R im, 3: RDS S0, 4: S1 (two tables)
                const uint4* src = blk == 0 ? bp_tab + (size_t)slot.x * kBpTabSlotU4 + within
                                 : (blk < 3 ? bp_tab + (size_t)slot.y * kBpTabSlotU4 + blk * 4 * kBpTabU4 + within : rds_tab + (blk - 3) * 4 * kBpTabU4 + within);
                reinterpret_cast<uint4*>(tabs)[j] = *src;
            }
        }
    }
    const int mode0 = (int)mixctl[2 * c], mode1 = two ? (int)mixctl[2 * c + 2] : 0;
    const float kmix0 = mixctl[2 * c + 1], kmix1 = two ? mixctl[2 * c + 3] : 0.0f;
    if (lmr_est_prev && est_wave) {
        float part = 0.0f;
#pragma unroll
        for (int k = 0; k < kLmrInlineMax / kWave; k++) part += ev[k];
        float nxt = fmaf(wave_sum_f32(part) * __builtin_amdgcn_rcpf((float)d.n_est), 0.1f, wv ? off_prev1 : off_prev0);
        const float two_pi = bits_f32(kTwoPiBits);
        nxt = (nxt >= two_pi) ? nxt - two_pi : ((nxt <= -two_pi) ? nxt + two_pi : nxt);
        if (lane == 0) { off_s[wv] = nxt; if (tile_first == 0) st(state, field_cur, d.C, c + wv) = nxt; }
    }
    // a block's first tile: S_old[m], m < 31 (reference: the FIR history holds samples mixed with the previous block's offset) — linear in the
    // window's first 188 samples: a fixed matrix (fp16: S_old is a correction, 2^-11 of it is 1e-6 of the output), 8 lanes per output
#pragma unroll
    for (int sx = 0; sx < SPW; sx++) {
      if (edge && (sx == 0 || two)) {
        if (sx) __syncthreads();         // (the first station's reads of the scratch)
        if (tid < 48) *reinterpret_cast<float4*>(wf32 + 4 * tid) = sx ? qe1 : qe;
        __syncthreads();
        if (tid < kBpEdgeRows) {
            const float* wp = wf32 + 24 * (tid & 7);
            float ar = 0.0f, ai = 0.0f;
            typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int k = 0; k < kBpEdgeU4; k++) {
                const float4 w4 = *reinterpret_cast<const float4*>(wp + 4 * k);
                const uint32_t ew[4] = {em[k].x, em[k].y, em[k].z, em[k].w};
                const float ws[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const h2_t e = __builtin_bit_cast(h2_t, ew[u]);
                    ar = fmaf((float)e[0], ws[u], ar); ai = fmaf((float)e[1], ws[u], ai);
                }
            }
            ar = oct_sum_f32(ar); ai = oct_sum_f32(ai);
            if ((tid & 7) == 0) s_old[sx][tid >> 3] = make_float2(ar, ai);
        }
      }
    }
    __syncthreads();                     // the tables, off_s, S_old: the workgroup's only barrier(s) — from here every wavefront is on its own
    if (lmr_est_prev) { off_cur0 = off_s[0]; if (SPW == 2 && two) off_cur1 = off_s[1]; }
    X_STAMP(1);

    // ---- wavefront w: tiles tile_first + w, + 4, ... — window, FIRs of all four families, outputs, nothing shared but the tables
    uint32_t* fh = win[wv];
    uint32_t* fl = fh + G::NBW;
    float4 qw[5];                        // a window = 303 quads: four per lane and quads 256 .. 302 (quad 303 lies behind the window: zeros — the tables' zero taps reach it)
    // (SPW == 2: a "tile" index runs over both stations' tiles, station = index / tiles)
    const int tiles_wg = two ? 2 * tiles : tiles;
    auto wload = [&](int tix) {
        const int sx = (SPW == 2 && tix >= tiles) ? 1 : 0, tile = tix - sx * tiles;
        const float* wsrc = fo_c0 + (size_t)sx * (kFoPad + n) + (4 * tile * TA - 188);                   // 16-byte aligned (rows and kFoPad are multiples of 4 floats)
#pragma unroll
        for (int r = 0; r < 4; r++) qw[r] = ld_mid(reinterpret_cast<const float4*>(wsrc + 4 * (lane + 64 * r)));
        const int q4 = 256 + lane;
        qw[4] = ld_mid(reinterpret_cast<const float4*>(wsrc + 4 * (q4 < G::WN / 4 ? q4 : G::WN / 4 - 1)));
    };
    if (tile_first + wv < tiles_wg) wload(tile_first + wv);
    for (int it = 0; it < nt; it++) {
        const int tix = tile_first + 4 * it + wv;
        if (tix >= tiles_wg) break;
        const int sx = (SPW == 2 && tix >= tiles) ? 1 : 0, tile = tix - sx * tiles, i0 = tile * TA;
        const int cc = c + sx;                                   // this tile's station
        const float4* po_c = po_c0 + (size_t)sx * (1 + n / kSpan);
        const float off_prev = sx ? off_prev1 : off_prev0, off_cur = sx ? off_cur1 : off_cur0, kmix = sx ? kmix1 : kmix0;
        const int mode = sx ? mode1 : mode0;
        // (the lane index, opaque to the optimiser from here on: left to itself it hoists whatever depends only on the lane out of the tile
        //  loop — two dozen registers that would live across the FIRs)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        __builtin_assume(ln >= 0 && ln < 64);
        const int lrow = ln & 15, lq = ln >> 4;
        // this lane's outputs: audio m0 .. m0 + 3, m0 = i0 + 16 lrow + 4 lq (accumulator rows 4 lq .. 4 lq + 3 of column lrow); RDS r0, r0 + 1,
        // r0 = i0 / 2 + 8 lrow + 2 lq.  Centres of their FIR windows: t_c = 4 m - 124 + 63.5, t_c = 8 r - 120 + 63.5 (analytic-sample time);
        // a lane's outputs lie in ONE span of 128 (2 t_c = 8 m - 121 = 7 (mod 32) for the first, + 24 for the last)
        const int m0 = i0 + 16 * lrow + 4 * lq, r0 = (i0 >> 1) + 8 * lrow + 2 * lq;
        const int tc2a = 8 * m0 - 121, tc2r = 16 * r0 - 113;

        // ---- the window: split into bf16 halves (x = hi + lo + O(2^-16 x)), two per word, 8 elements of padding after every 32
        {
            auto put = [&](int q, const float4& v) {
                uint32_t h0, l0, h1, l1, h2, l2, h3, l3;
                split_bf16(v.x, h0, l0); split_bf16(v.y, h1, l1); split_bf16(v.z, h2, l2); split_bf16(v.w, h3, l3);
                const int w = G::pad(4 * q) >> 1;
                *reinterpret_cast<uint2*>(fh + w) = make_uint2(pack_hi16(h0, h1), pack_hi16(h2, h3));
                *reinterpret_cast<uint2*>(fl + w) = make_uint2(pack_hi16(l0, l1), pack_hi16(l2, l3));
            };
#pragma unroll
            for (int r = 0; r < 4; r++) put(ln + 64 * r, qw[r]);
            if (ln < G::WNP / 4 - 256) put(256 + ln, (256 + ln >= G::WN / 4) ? make_float4(0.f, 0.f, 0.f, 0.f) : qw[4]);
        }
        const float4 pva = po_c[tc2a >> 8], pvr = po_c[tc2r >> 8];          // the span cubics: asked for now, needed behind the FIRs
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                  // (the window is this wavefront's own: its writes are in place, no barrier)
        __builtin_amdgcn_wave_barrier();
        X_STAMP(0);

        // ---- the FIRs: four families and S1 on the same window operands; three products per tap (hi hi, lo hi, hi lo) into ONE fp32 accumulator per
        //      family — the four families interleaved, a family's products are four matrix instructions apart
        f32x4 acc[4] = {kZero4, kZero4, kZero4, kZero4}, s1 = kZero4;
        {
            // this lane's operands: window elements 64 lrow + 32 k + 8 lq .. + 7 = word wb + 20 k; taps: row lrow of a family's block (copy 4 / the
            // imaginary rail for odd rows), K-step k 32 elements on
            const int wb = G::pad(64 * lrow + 8 * lq) >> 1;
            const uint16_t* ta = tabs + (lrow & 1) * kBpTL + kBpPadL + 8 * lq - 4 * (lrow & ~1);                 // families 0 .. 2: + 4 f TL (0: taps 32 into the window)
            const uint16_t* t3 = tabs + (12 + (lrow & 1)) * kBpTL + kBpPadL + 8 * lq - 8 * (lrow >> 1);          // RDS S0; S1 = + 4 TL
            auto ld = [](const void* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p)); };
#pragma unroll
            for (int sK = 0; sK < G::KS; sK++) {
                const bf16x8 bh = ld(fh + wb + 20 * sK), bl = ld(fl + wb + 20 * sK);
                bf16x8 ah[4], al[4];
                ah[0] = ld(ta - 32 + 32 * sK);               al[0] = ld(ta - 32 + 2 * kBpTL + 32 * sK);
                ah[1] = ld(ta + 4 * kBpTL + 32 * sK);        al[1] = ld(ta + 6 * kBpTL + 32 * sK);
                ah[2] = ld(ta + 8 * kBpTL + 32 * sK);        al[2] = ld(ta + 10 * kBpTL + 32 * sK);
                ah[3] = ld(t3 + 32 * sK);                    al[3] = ld(t3 + 2 * kBpTL + 32 * sK);
                const bf16x8 a1 = ld(t3 + 4 * kBpTL + 32 * sK);
#pragma unroll
                for (int f = 0; f < 4; f++) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[f], bh, acc[f], 0, 0, 0);
#pragma unroll
                for (int f = 0; f < 4; f++) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[f], bh, acc[f], 0, 0, 0);
#pragma unroll
                for (int f = 0; f < 4; f++) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[f], bl, acc[f], 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bh, s1, 0, 0, 0);
                // (left alone the scheduler hoists every K-step's LDS reads in front of the first product: 350 registers)
#ifndef FMD_BP_SB
#define FMD_BP_SB 1
#endif
                if ((sK % FMD_BP_SB) == FMD_BP_SB - 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
        asm volatile("" ::: "memory");                                      // (the next window's writes stay behind these reads)
        X_STAMP(2);
        // the next tile's window: asked for now, split and stored at the top of the next iteration — an epilogue from here
        if (it + 1 < nt && tix + 4 < tiles_wg) wload(tix + 4);

        // ---- outputs from the accumulators as they lie: the rotation, a15 MixAudio (reference :549-585), the phase estimate (:500-510)
        {
            // NCO deviation at a window's centre: the span's cubic p(u), u = t_c within its span (x.5); carrier at the window's first sample:
            // -H 19 (t0 + 1) / 128, t0 + 1 = 4 (m + 1) - 127
            const float uc0 = 0.5f * (float)(tc2a & 255);
            float dc = 0.0f, ds = 0.0f;
            if (tile == 0) {             // S + (e^{j 2 pi (off_prev - off_cur)} - 1) S_old on the block's first 31 outputs
                const float dph = off_prev - off_cur;
                dc = fast_cos_turns(dph) - 1.0f; ds = fast_sin_turns(dph);
            }
            float lmr_v[4], lre_v[4], lpr_v[4], au[8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int m = m0 + i;
                const float uc = uc0 + 4.0f * (float)i;
                const float p = fmaf(fmaf(fmaf(pva.w, uc, pva.z), uc, pva.y), uc, pva.x);
                const float nom = (float)((-38 * (4 * (m + 1) - 127)) & 127) * (1.0f / 128.0f);      // the carrier's phase mod one turn, reduced in integers (exact for any block length)
                float2 sv = make_float2(acc[1][i], acc[2][i]);
                if (tile == 0 && 16 * lrow + 4 * lq + i < 31) {
                    const float2 so = s_old[sx][16 * lrow + 4 * lq + i];
                    sv.x += fmaf(dc, so.x, -(ds * so.y)); sv.y += fmaf(dc, so.y, ds * so.x);
                }
                const float ph = fmaf(2.0f, p, nom) + off_cur;
                const float cs = fast_cos_turns(ph), sn = fast_sin_turns(ph);
                const float lmr_re = fmaf(sv.x, cs, -(sv.y * sn)), lmr = fmaf(sv.x, sn, sv.y * cs);
                const float lpr = acc[0][i];
                float l, r;
                if (mode == FMD_AUDIO_STEREO) { l = fmaf(lmr, kmix, lpr); r = fmaf(-lmr, kmix, lpr); }
                else if (mode == FMD_AUDIO_LMR) { l = lmr; r = lmr; }
                else { l = lpr; r = lpr; }
                au[2 * i] = l + l; au[2 * i + 1] = r + r;
                lmr_v[i] = lmr; lre_v[i] = lmr_re; lpr_v[i] = lpr;
            }
            float4* ap = reinterpret_cast<float4*>(audio + 2 * ((size_t)cc * d.n_audio + m0));       // four frames: 32 bytes, aligned
            st_stream(ap, make_float4(au[0], au[1], au[2], au[3])); st_stream(ap + 1, make_float4(au[4], au[5], au[6], au[7]));
            if (keep_taps) {
                *reinterpret_cast<float4*>(lpr_out + (size_t)cc * d.n_audio + m0) = make_float4(lpr_v[0], lpr_v[1], lpr_v[2], lpr_v[3]);
                *reinterpret_cast<float4*>(lmr_out + (size_t)cc * d.n_audio + m0) = make_float4(lmr_v[0], lmr_v[1], lmr_v[2], lmr_v[3]);
            }
            // reference :500-510: estimate against the +-pi/2 constellation, every 10th output of the block — at most one of a lane's four
            {
                const int k10 = (10 - m0 % 10) % 10;                        // m0 + k10 is the next multiple of 10
                if (k10 < 4) {
                    const float a = k10 == 0 ? lmr_v[0] : (k10 == 1 ? lmr_v[1] : (k10 == 2 ? lmr_v[2] : lmr_v[3]));
                    const float b = k10 == 0 ? lre_v[0] : (k10 == 1 ? lre_v[1] : (k10 == 2 ? lre_v[2] : lre_v[3]));
                    const float pe = fast_atan2f(a, b);
                    const float half_pi = bits_f32(kHalfPiBits);
                    lmr_est[(size_t)cc * d.n_est + (m0 + k10) / 10] = (pe > 0.0f) ? (half_pi - pe) : (-half_pi - pe);
                }
            }
            // a12 + a13: the RDS baseband, y = e^{j 2 pi (3 p(t_c) + nom)} (S0 + j 2 pi 3 p'(t_c) S1) — accumulator rows (o, rail) = this lane's two
            // outputs; the AGC's block power (reference agc.h:21-30) as two partial sums per tile
            {
                const float ur0 = 0.5f * (float)(tc2r & 255);
                float y[4], pw[2];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int ri = r0 + j;
                    const float ur = ur0 + 8.0f * (float)j;
                    const float pr = fmaf(fmaf(fmaf(pvr.w, ur, pvr.z), ur, pvr.y), ur, pvr.x);
                    const float dpr = fmaf(fmaf(3.0f * pvr.w, ur, 2.0f * pvr.z), ur, pvr.y);                      // turns per sample
                    const float nomr = (float)((-57 * (8 * (ri + 1) - 127)) & 127) * (1.0f / 128.0f);
                    const float eps = bits_f32(kTwoPiBits) * 3.0f * dpr;
                    const float xr = fmaf(-eps, s1[2 * j + 1], acc[3][2 * j]), xi = fmaf(eps, s1[2 * j], acc[3][2 * j + 1]);
                    const float phr = fmaf(3.0f, pr, nomr);
                    const float cr = fast_cos_turns(phr), sr = fast_sin_turns(phr);
                    y[2 * j] = fmaf(xr, cr, -(xi * sr)); y[2 * j + 1] = fmaf(xr, sr, xi * cr);
                    pw[j] = wave_sum_f32(fmaf(y[2 * j], y[2 * j], y[2 * j + 1] * y[2 * j + 1]));
                }
                *reinterpret_cast<float4*>(rds + (size_t)cc * d.n_rds + r0) = make_float4(y[0], y[1], y[2], y[3]);
                if (ln == 0) *reinterpret_cast<float2*>(rds_pow + ((size_t)cc * tiles + tile) * 2) = make_float2(pw[0], pw[1]);
            }
        }
        X_STAMP(3);
        X_STAMP(4);
    }
#ifdef FMD_X_PROBE
    if (xp_on && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) == 0) { atomicAdd(&g_x_probe2[7], __builtin_readcyclecounter() - xp_c0); atomicAdd(&g_x_probe2[15], wall_clock64() - xp_w0); }
#endif
}
