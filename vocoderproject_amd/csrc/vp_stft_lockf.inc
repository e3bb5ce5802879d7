// vp_stft_lockf.inc -- the peak-locked phase-vocoder kernels with SUB-BIN region offsets (included by vp_stft.hip behind
// vp_stft_lock.inc: its carve, masks, pv_lock_nearest, pv_lock_bin and pv_lock_turn).
//
// The locked stage moves a peak's region by the integer floor(P r + 0.5) - P while its angle advances at the true frequency: the lobe
// sits up to half a bin, plus the peak's own sub-bin position, from the frequency its phase turns at, and successive frames do not add
// up in the overlap-add (a 0.5 tone leaves at 0.38).  Here (Laroche & Dolson's remedy; the definition is tests/pv_lockf_reference.py)
// the peak's centre c = P + delta is the vertex of the parabola through its three linear magnitudes, the region is translated by the
// real-valued D = c (r - 1), and the spectrum is interpolated at u = kk - D with six taps of a Hann-tapered sinc,
//
//     Y[kk] = exp(2 pi i th[P]) sum_j w_j (-1)^(kk - k_j) X[k_j],   k_j = floor(u) + j,  j = -2 .. 3,  own[k_j] == P.
//
// With f = u - floor(u): sinc(f - j) = (-1)^j sin(pi f) / (pi (f - j)), and (-1)^(kk - k_j) = (-1)^(kk - floor(u)) (-1)^j, so the two
// alternations cancel and what is left per bin is ONE sign, ONE sin(pi f), and per tap the taper over f - j.  The taper's angle
// pi (f - j) / 3 is pi f / 3 less a constant: one sincos and angle addition.  The six 1 / (f - j) come from one division (prefix and
// suffix products).  f == 0 is the single tap of weight 1 (the identity at r = 1, where D is exactly 0).
//
// vp_k_stft_pv_lockf and vp_k_pv_stream_lockf are WRITTEN-OUT COPIES of vp_k_stft_pv_lock and vp_k_pv_stream_lock (docs/HISTORY.md, "One
// phase-vocoder stage for both kernels", for why copies): framing, transforms, ratio table, overlap-add, state record and bookkeeping are
// the parents', statement for statement.  What differs is marked "lockf:".
//
// State: as the parents' (phPrev, theta in PvLds::sum), so sub-bin, locked, curve, plain and formant calls may follow each other on one
// streaming handle; after a change of kind the output is defined and finite but carries a phase jump.
//
// lockf: LDS is the parents', byte for byte.  D of a peak P < N lies in the wavefront's `inc` row at P + 1: peaks are at least three bins
// apart, so the slot is no peak's, and pv_lock_turn reads the row at peaks only.  P == N has delta = 0 and D = N (r - 1), formed where
// it is used.

// lockf: pv_lock_plan with the peak's offset: own[e], pk[e] as there; src[e] is 0 where synthesis bin e has a region (a shifted peak is
// left), else -1 (zero).  The parabola's three magnitudes are read before the row is overwritten: a peak's neighbours are no peaks, so
// only this lane writes P and P + 1.
__device__ __forceinline__ bool pv_lockf_plan(const PvLds &pv, const PvLockLds &lk, int wv, int prevSlot, int ln, bool lane0, double ratio, double invO, int O,
                                              int (&own)[9], int (&src)[9], int (&pk)[9])
{
    constexpr int N = 512, nb = N + 1;
    lds_f64 *mrow = pv.inc + wv * nb;
    unsigned long long bal[9];
    bool isPk[9];
#pragma unroll
    for (int e = 0; e < 9; e++) {
        const int k = pv_lock_bin(e, ln);
        const double c = mrow[k];
        const double l1 = mrow[max(k - 1, 0)], l2 = mrow[max(k - 2, 0)], r1 = mrow[min(k + 1, N)], r2 = mrow[min(k + 2, N)];
        bool p = (e < 8 || lane0) && c > 0.0;
        p = p && (k < 1 || c > l1) && (k < 2 || c > l2) && (k + 1 > N || c >= r1) && (k + 2 > N || c >= r2);
        isPk[e] = p;
        bal[e] = __ballot(p);
    }
    unsigned long long any = 0ull;
#pragma unroll
    for (int e = 0; e < 9; e++) any |= bal[e];
#pragma unroll
    for (int e = 0; e < 9; e++) { own[e] = 0; src[e] = -1; pk[e] = 0; }
    if (any == 0ull) return false;                                             // (all zeros, or nothing finite: the frame is silent)
    pv_lock_mask(lk.peaks, bal, lane0);
#pragma unroll
    for (int e = 0; e < 9; e++) if (e < 8 || lane0) lk.back[pv_lock_bin(e, ln)] = -1;
    wave_sync();                                                               // (and every lane has read its magnitudes)
#pragma unroll
    for (int e = 0; e < 9; e++) {
        if (!isPk[e]) continue;
        const int k = pv_lock_bin(e, ln);
        // lockf: the centre of the peak and its region's offset
        if (k < N) {
            double delta = 0.0;
            if (k > 0) {
                const double a = mrow[k - 1], c = mrow[k], b = mrow[k + 1];
                delta = fmin(fmax(0.5 * (a - b) / (a - 2.0 * c + b), -0.5), 0.5);
            }
            mrow[k + 1] = ((double)k + delta) * (ratio - 1.0);
        }
        double d = pv.phPrev[(wv + 1) * nb + k] - pv.phPrev[prevSlot * nb + k] - (double)k * invO;
        d -= rint(d);
        const double nu = (double)k + d * (double)O;
        mrow[k] = (nu * (ratio - 1.0)) * invO;                                 // r - 1 is exact on [0.5, 2], 1 / O a power of two
        const int kp = (int)floor((double)k * ratio + 0.5);
        if (kp <= N) lk.back[kp] = k;                                          // (peaks are three bins apart: distinct for r >= 0.5)
    }
    wave_sync();
#pragma unroll
    for (int e = 0; e < 9; e++) {
        const int k = pv_lock_bin(e, ln);
        bal[e] = __ballot((e < 8 || lane0) && lk.back[k] >= 0);
        own[e] = pv_lock_nearest(lk.peaks, k);
        if (e < 8 || lane0) lk.own[k] = own[e];
    }
    any = 0ull;
#pragma unroll
    for (int e = 0; e < 9; e++) any |= bal[e];
    pv_lock_mask(lk.moved, bal, lane0);
    wave_sync();
    if (any != 0ull) {
#pragma unroll
        for (int e = 0; e < 9; e++) {
            const int kk = pv_lock_bin(e, ln);
            const int ps = pv_lock_nearest(lk.moved, kk);
            pk[e] = lk.back[ps];
            src[e] = 0;                                                        // lockf: the taps are chosen in the gather
        }
    }
    return true;
}

// lockf: the interpolating gather: synthesis bin e of the lane is the six-tap interpolation of the wavefront's spectrum at kk - D over
// the bins its peak owns, rotated by th[e]; or zero
__device__ __forceinline__ void pv_lockf_gather(const PvLds &pv, const PvLockLds &lk, int wv, int ln, bool lane0, double ratio, const int (&src)[9],
                                                const int (&pk)[9], const double (&th)[9], RPairs &X)
{
    constexpr int N = 512, nb = N + 1;
    // cos and sin of pi j / 3, j = -2 .. 3
    constexpr double H3 = 0.8660254037844386;
    constexpr double CJ[6] = {-0.5, 0.5, 1.0, 0.5, -0.5, -1.0}, SJ[6] = {-H3, -H3, 0.0, H3, H3, 0.0};
#pragma unroll
    for (int e = 0; e < 9; e++) {
        if (e == 8 && !lane0) continue;
        double re = 0.0, im = 0.0;
        if (src[e] >= 0) {
            const int kk = pv_lock_bin(e, ln), pa = pk[e];
            const double D = pa < N ? pv.inc[wv * nb + pa + 1] : (double)N * (ratio - 1.0);
            const double u = (double)kk - D, uf = floor(u), f = u - uf;        // |u| < 1024
            const int u0 = (int)uf;
            double w[6] = {0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
            if (f != 0.0) {
                double s1, c1, s3, c3;
                pv_sincos_turns(0.5 * f, s1, c1);                              // sin(pi f)
                pv_sincos_turns(f * (1.0 / 6.0), s3, c3);                      // (sin, cos)(pi f / 3)
                double a[6], pre[6], run = 1.0;
#pragma unroll
                for (int j = 0; j < 6; j++) { a[j] = f - (double)(j - 2); pre[j] = run; run *= a[j]; }
                double suf = 0.3183098861837907 * s1 / run;                    // sin(pi f) / pi over the product of all six
#pragma unroll
                for (int j = 5; j >= 0; j--) {
                    // taper 1/2 + 1/2 cos(pi (f - j) / 3) by angle addition
                    w[j] = (0.5 + 0.5 * __builtin_fma(c3, CJ[j], s3 * SJ[j])) * (pre[j] * suf);
                    suf *= a[j];
                }
            }
            double ar = 0.0, ai = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const int kj = u0 + j - 2;
                if (kj >= 0 && kj <= N && lk.own[kj] == pa) {
                    const d2 x = pv.ana[kj];
                    ar = __builtin_fma(w[j], x.x, ar);
                    ai = __builtin_fma(w[j], x.y, ai);
                }
            }
            if ((kk - u0) & 1) { ar = -ar; ai = -ai; }                         // the one sign left of (-1)^(kk - k_j) and the sinc's own
            double sn, cs;
            pv_sincos_turns(th[e], sn, cs);
            re = __builtin_fma(ar, cs, -(ai * sn));
            im = __builtin_fma(ar, sn, ai * cs);
        }
        if (e == 8) { X.hr = re; X.hi = im; }
        else if (e & 1) { X.mr[e >> 1] = re; X.mi[e >> 1] = im; }
        else { X.kr[e >> 1] = re; X.ki[e >> 1] = im; }
    }
    if (lane0) { X.ki[0] = 0.0; X.mi[0] = 0.0; }
}

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv_lockf(VpStftArgs A, const double *ratioTab)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 512;                                                     // complex points = F / 2
    const int F = A.F, hop = A.hop, O = A.O, T = A.T;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;                             // [(O - 1) hop]
    const PvLds pv = pv_lds_carve((lds_f64 *)smem + stft_lds_base(F, hop) / 8, wv);
    const PvLockLds lk = pv_lock_carve((lds_f64 *)smem + (stft_lds_base(F, hop) + pv_lds_bytes()) / 8, wv);
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)((stft_lds_base(F, hop) + pv_lds_bytes() + pv_lock_lds_bytes()) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif

    FftLane L;
    fft_lane_init(L, lane, A.tw1, A.tw2);
    d2 wa[8];                                                                  // (w[2n], w[2n + 1]), n = lane + 64 r
    d2 ws[4];                                                                  // W_1024^(64 q + lane)
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
#pragma unroll
    for (int q = 0; q < 4; q++) ws[q] = ((const d2 *)A.tws)[lane * 4 + q];
    const bool lane0 = lane == 0;

    for (int i = tid; i < F - hop; i += 64 * NWV) carry[i] = 0.f;
    for (int i = tid; i < VP_PV_NB; i += 64 * NWV) { pv.phPrev[i] = 0.0; pv.sum[i] = 0.0; }
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * T;
    const double *rs = ratioTab + (size_t)s * A.nFrames;
    // the frame's samples, and its ratio, are requested a round ahead
    f2 xv[8];
    double rq = 1.0;
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) { stft_load_frame(xv, xs + (size_t)f_ * hop, A.aligned, lane); rq = rs[f_]; }
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        C8 z;
        RPairs X;
        const double ratio = pv_curve_clamp(rq);
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) { z.re[r] = (double)xv[r].x * wa[r].x; z.im[r] = (double)xv[r].y * wa[r].y; }
        }
        request(rd + 1);
        if (live) {
            fft512_rx(z, xb, L);
            rfft_split(z, xb, lane, (const d2 *)ws, X);
        }
        {
            // ---- the peak-locked stage, phases in TURNS (to the merge)
            const int nb = N + 1;
            const double invO = 1.0 / (double)O;
            // (the lane number through a register the compiler cannot see through: vp_k_stft_pv2k)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            if (live) {
                // spectrum, magnitude and phase of the lane's bins, straight to LDS
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k = 64 * q + ln, m = N - k;
                    pv.ana[k] = d2{X.kr[q], X.ki[q]}; pv.ana[m] = d2{X.mr[q], X.mi[q]};
                    pv.inc[wv * nb + k] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); pv.phPrev[(wv + 1) * nb + k] = pv_phase_turns(X.ki[q], X.kr[q]);
                    pv.inc[wv * nb + m] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); pv.phPrev[(wv + 1) * nb + m] = pv_phase_turns(X.mi[q], X.mr[q]);
                }
                if (lane0) {
                    pv.ana[N / 2] = d2{X.hr, X.hi};
                    pv.inc[wv * nb + N / 2] = sqrt(X.hr * X.hr + X.hi * X.hi); pv.phPrev[(wv + 1) * nb + N / 2] = pv_phase_turns(X.hi, X.hr);
                }
            }
            __syncthreads();
            int own[9], src[9], pk[9];
            bool has = false;
            if (live) has = pv_lockf_plan(pv, lk, wv, wv, ln, lane0, ratio, invO, O, own, src, pk);   // lockf:
            // theta is handed through the round in frame order, in place
            double th[9];
#pragma unroll
            for (int e = 0; e < 9; e++) th[e] = 0.0;
#pragma unroll
            for (int w = 0; w < NWV; w++) {
                if (w > 0) __syncthreads();
                if (live && has && wv == w) pv_lock_turn(pv, wv, ln, lane0, own, src, pk, th);
            }
            if (live) pv_lockf_gather(pv, lk, wv, ln, lane0, ratio, src, pk, th, X);                  // lockf:
            // (every live wavefront is past its reads of the previous frame's phases: the turns' barriers, or program order when the
            // round's only live wavefront is wavefront 0)
            const int lastLive = min(NWV - 1, A.nFrames - 1 - rd * NWV);
            if (live && wv == lastLive) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k = pv_lock_bin(e, ln);
                    pv.phPrev[k] = pv.phPrev[(wv + 1) * nb + k];
                }
            }
            // ---- end of the stage
        }
        lds_f2 *slot = (lds_f2 *)(slots + wv * 2048);
        if (live) {
            rfft_merge_conj(z, xb, lane, (const d2 *)ws, X, A.c);
            fft512_rx(z, xb, L);
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{(float)(z.re[r] * wa[r].x), (float)(-(z.im[r] * wa[r].y))};
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{0.f, 0.f};
        }
        __syncthreads();
        stft_overlap_add(A, slots, carry, s, rd, rd >= R.rFirst, tid);
        __syncthreads();
    }
}

// ---- streaming: vp_k_pv_stream_lock with the sub-bin stage.  theta is the record's second array, handed from the call's first live frame
// to its last whatever their wavefronts.  The call's bookkeeping is the pv_call_* helpers of vp_stft.hip.
__global__ __launch_bounds__(64 * NWV) void vp_k_pv_stream_lockf(VpPvArgs A, const double *ratioTab)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x;
    constexpr int N = 512, F = 1024, nb = N + 1;
    const int hop = A.hop, O = A.O, NB = A.N, S = A.S;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *ring = (lds_f32 *)smem + NWV * 2048;                              // [VP_PV_RING]
    lds_f32 *hist = ring + VP_PV_RING;                                         // [F]
    const PvLds pv = pv_lds_carve((lds_f64 *)(hist + F), wv);
    const PvLockLds lk = pv_lock_carve((lds_f64 *)smem + pv_stream_lds_bytes() / 8, wv);
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)((pv_stream_lds_bytes() + pv_lock_lds_bytes()) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif
    unsigned char *rec = A.state + (size_t)s * VP_PV_REC_BYTES;
    double *recD = (double *)rec;
    float *recHist = (float *)(rec + VP_PV_HIST_BYTES), *recCarry = (float *)(rec + VP_PV_CARRY_BYTES);

    double recRatio = recD[VP_PV_RATIO];                                       // written back, not used
    long long n = ((const long long *)recD)[VP_PV_COUNT];
    const bool rst = pv_scan_updates(A, s, recRatio);
    if (rst) n = 0;
    const PvCall C = pv_call_geometry(n, A.nBlocks * NB, hop, A.L);
    const int nf = C.nf;

    pv_call_load_hist(C, hist, recHist, tid);
    for (int i = tid; i < nb; i += 64 * NWV) { pv.phPrev[i] = rst ? 0.0 : recD[i]; pv.sum[i] = rst ? 0.0 : recD[nb + i]; }
    pv_call_load_ring(C, ring, recCarry, rst, tid);

    FftLane Lf;
    fft_lane_init(Lf, lane, A.tw1, A.tw2);
    d2 wa[8];
    d2 ws[4];
#pragma unroll
    for (int r = 0; r < 8; r++) wa[r] = ((const d2 *)A.win)[lane + 64 * r];
#pragma unroll
    for (int q = 0; q < 4; q++) ws[q] = ((const d2 *)A.tws)[lane * 4 + q];
    const bool lane0 = lane == 0;
    __syncthreads();

    const float *xs = A.in + (size_t)s * NB;
    float *ys = A.out + (size_t)s * NB;
    const int nRounds = pv_call_rounds(C);
    int cb = C.er;
    f2 xv[8];
    double rq = 1.0;
    auto request = [&](int k_) {
        const int fr_ = C.fr0 + NWV * k_ + wv;
        if (k_ < nRounds && fr_ >= 0 && fr_ < nf) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int rel = fr_ * hop + 2 * (lane + 64 * r);
                xv[r] = f2{pv_call_sample(C, hist, xs, NB, S, rel), pv_call_sample(C, hist, xs, NB, S, rel + 1)};
            }
            const unsigned blk = (unsigned)(fr_ * hop + F - 1 - C.H) / (unsigned)NB; // the block in which the frame's last sample arrives
            rq = ratioTab[(size_t)blk * S + s];
        }
    };
    request(0);
    for (int k = 0; k < nRounds; k++) {
        const int frW0 = C.fr0 + NWV * k;
        const int fr = frW0 + wv;
        const bool live = fr >= 0 && fr < nf;                                  // (wavefront-uniform)
        const int wFirst = max(0, -frW0), wLast = min(NWV - 1, nf - 1 - frW0);
        C8 z;
        RPairs X;
        const double ratio = pv_curve_clamp(rq);
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) { z.re[r] = (double)xv[r].x * wa[r].x; z.im[r] = (double)xv[r].y * wa[r].y; }
        }
        request(k + 1);
        if (live) {
            fft512_rx(z, xb, Lf);
            rfft_split(z, xb, lane, (const d2 *)ws, X);
        }
        {
            // ---- the peak-locked stage (vp_k_stft_pv_lockf's), to the merge
            const double invO = 1.0 / (double)O;
            const int prevSlot = wv == wFirst ? 0 : wv;
            int ln = lane;
            asm volatile("" : "+v"(ln));
            if (live) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k_ = 64 * q + ln, m = N - k_;
                    pv.ana[k_] = d2{X.kr[q], X.ki[q]}; pv.ana[m] = d2{X.mr[q], X.mi[q]};
                    pv.inc[wv * nb + k_] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); pv.phPrev[(wv + 1) * nb + k_] = pv_phase_turns(X.ki[q], X.kr[q]);
                    pv.inc[wv * nb + m] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); pv.phPrev[(wv + 1) * nb + m] = pv_phase_turns(X.mi[q], X.mr[q]);
                }
                if (lane0) {
                    pv.ana[N / 2] = d2{X.hr, X.hi};
                    pv.inc[wv * nb + N / 2] = sqrt(X.hr * X.hr + X.hi * X.hi); pv.phPrev[(wv + 1) * nb + N / 2] = pv_phase_turns(X.hi, X.hr);
                }
            }
            __syncthreads();
            int own[9], src[9], pk[9];
            bool has = false;
            if (live) has = pv_lockf_plan(pv, lk, wv, prevSlot, ln, lane0, ratio, invO, O, own, src, pk);   // lockf:
            // theta continues from the state at the call's first live frame and is left by its last
            double th[9];
#pragma unroll
            for (int e = 0; e < 9; e++) th[e] = 0.0;
#pragma unroll
            for (int w = 0; w < NWV; w++) {
                if (w > 0) __syncthreads();
                if (live && has && wv == w) pv_lock_turn(pv, wv, ln, lane0, own, src, pk, th);
            }
            if (live) pv_lockf_gather(pv, lk, wv, ln, lane0, ratio, src, pk, th, X);                        // lockf:
            if (live && wv == wLast) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k_ = pv_lock_bin(e, ln);
                    pv.phPrev[k_] = pv.phPrev[(wv + 1) * nb + k_];
                }
            }
            // ---- end of the stage
        }
        lds_f2 *slot = (lds_f2 *)(slots + wv * 2048);
        if (live) {
            rfft_merge_conj(z, xb, lane, (const d2 *)ws, X, A.c);
            fft512_rx(z, xb, Lf);
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f2{(float)(z.re[r] * wa[r].x), (float)(-(z.im[r] * wa[r].y))};
        }
        __syncthreads();
        cb = pv_call_round_tail(C, ring, slots, ys, NB, S, hop, frW0, wFirst, wLast, cb, tid);
        __syncthreads();
    }
    pv_call_emit(C, ring, ys, NB, S, cb, C.er + C.M, tid);                     // the flush

    pv_call_store_hist(C, recHist, hist, xs, NB, S, hop, tid);
    pv_call_store_carry(C, recCarry, ring, tid);
    __syncthreads();
    for (int i = tid; i < nb; i += 64 * NWV) { recD[i] = pv.phPrev[i]; recD[nb + i] = pv.sum[i]; }
    if (tid == 0) { recD[VP_PV_RATIO] = recRatio; ((long long *)recD)[VP_PV_COUNT] = C.R; }
}

hipError_t vp_stft_lockf_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_stft_pv_lockf, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

size_t vp_stft_lockf_lds_bytes(int hop) { return vp_stft_lock_lds_bytes(hop); }                       // lockf: no row of its own
size_t vp_pv_lockf_lds_bytes() { return vp_pv_lock_lds_bytes(); }

hipError_t vp_stft_launch_lockf(const VpStftArgs &a, const double *d_ratio, int nStreams, hipStream_t st)
{
    const dim3 grid(1, nStreams), block(64 * NWV);                             // (one run: theta is a recurrence over the stream's frames)
    hipLaunchKernelGGL(vp_k_stft_pv_lockf, grid, block, vp_stft_lockf_lds_bytes(a.hop), st, a, d_ratio);
    return hipGetLastError();
}

hipError_t vp_pv_lockf_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_pv_stream_lockf, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_pv_launch_lockf(const VpPvArgs &a, const double *d_ratio, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_pv_stream_lockf, dim3(a.S), dim3(64 * NWV), vp_pv_lockf_lds_bytes(), st, a, d_ratio);
    return hipGetLastError();
}
