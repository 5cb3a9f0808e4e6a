// The body of hfg_unit_kernel and hfg_unit_cap_kernel (hifigan.hip), included into both: template parameters C, HI and the argument record `a`
// (HfgUnitArgs; a.m = the rows to work on) are in scope.  One text, so the two kernels cannot drift apart; textual rather than a shared inlined
// function because the exact kernel's register allocation moves when its body is inlined from a function (DESIGN 6c).
    using G = HfgGeo<C / 16>;
    constexpr int TM = G::TM, TN = G::TN, WN = G::WN, LDT = G::LDT, LD = C / 32, BM = 112;
    extern __shared__ __attribute__((aligned(1024))) u8 hfg_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN, r16 = lane & 15, kq = lane >> 4;
    const int h2 = (a.kr - 1) / 2, h1 = h2 * a.dil, RIN = 128 + 2 * h1;
    const int m0 = blockIdx.x * BM, t0 = m0 - h2, n0 = wn * TN * 16;
    u8* tin = hfg_smem;
    u8* txt = hfg_smem + (size_t)RIN * LD * 128;
    hfg_load_tile(a.xp, LD, a.m, t0 - h1, RIN, 0, LD, tin, tid);
    int lo[TM], hi[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) hfg_bounds(a.frame_utt, a.utt_off, a.rate, a.m, t0 + (wm * TM + tm) * 16 + r16, lo[tm], hi[tm]);
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    for (int j = 0; j < a.kr; ++j) {
        const int shift = (j - h2) * a.dil;
        int arow[TM];
        unsigned ok = 0u;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int r = (wm * TM + tm) * 16 + r16, g = t0 + r + shift;
            arow[tm] = r + j * a.dil;
            ok |= (g >= lo[tm] && g < hi[tm]) ? (1u << tm) : 0u;
        }
        hfg_tap<TM, TN, HI>(tin, RIN, LD, arow, ok, TM, a.w1p + ((size_t)j * C + n0 + r16) * LD * 64 + kq * 8, LD, kq, acc);
    }
    // LeakyReLU(intermediate) -> LDS as planes in the tile layout
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int col = n0 + tn * 16 + (lane & 15);
            const float b = a.b1[col];
            const int c = col >> 5, piece = (col & 31) >> 3, el = (col & 7) * 2;
            f32x4 v;  // this lane's four rows of the column, split by the one split every producer uses (what the two-launch form writes to tp)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = hfg_lrelu(acc[tm][tn][r] + b, a.slope);
            uint2 h, l;
            split4(v, h, l);
            const unsigned hw[2] = {h.x, h.y}, lw[2] = {l.x, l.y};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (wm * TM + tm) * 16 + (lane >> 4) * 4 + r, sw = (row >> 1) & 7;
                u8* line = txt + (size_t)(c * 128 + row) * 128;
                *reinterpret_cast<u16*>(line + ((piece ^ sw) << 4) + el) = (u16)(hw[r >> 1] >> ((r & 1) * 16));
                if (!HI) *reinterpret_cast<u16*>(line + (((4 + piece) ^ sw) << 4) + el) = (u16)(lw[r >> 1] >> ((r & 1) * 16));
            }
            acc[tm][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) hfg_bounds(a.frame_utt, a.utt_off, a.rate, a.m, m0 + (wm * TM + tm) * 16 + r16, lo[tm], hi[tm]);
    __syncthreads();
    const int tm_end = BM / 16 - wm * TM;  // row tile 7 of the 128 is not an output
    for (int j = 0; j < a.kr; ++j) {
        int arow[TM];
        unsigned ok = 0u;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int r = (wm * TM + tm) * 16 + r16, g = m0 + r + j - h2;
            arow[tm] = min(r + j, 127);  // (only skipped row tiles reach the clamp)
            ok |= (g >= lo[tm] && g < hi[tm]) ? (1u << tm) : 0u;
        }
        hfg_tap<TM, TN, HI>(txt, 128, LD, arow, ok, tm_end, a.w2p + ((size_t)j * C + n0 + r16) * LD * 64 + kq * 8, LD, kq, acc);
    }
    float* zt = reinterpret_cast<float*>(tin);  // every wave left the operand tile at the barrier above
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            if (tm >= tm_end) continue;
            const int col = n0 + tn * 16 + (lane & 15);
            const float b = a.b2[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) zt[((wm * TM + tm) * 16 + (lane >> 4) * 4 + r) * LDT + col] = acc[tm][tn][r] + b;
        }
    __syncthreads();
    for (int i = tid; i < BM * (C / 4); i += 256) {
        const int r = i / (C / 4), c4 = (i - r * (C / 4)) * 4;
        if (m0 + r >= a.m) continue;
        hfg_store4(a.e, m0 + r, C, c4, *reinterpret_cast<const f32x4*>(zt + r * LDT + c4));
    }
