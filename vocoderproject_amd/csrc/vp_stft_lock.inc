// vp_stft_lock.inc -- the phase-vocoder kernels with PEAK LOCKING (included by vp_stft.hip behind vp_stft_curve.inc: its helpers, tables,
// carves and pv_curve_clamp).
//
// The plain stage moves every bin on its own and runs one phase accumulator per synthesis bin: a sinusoid's main lobe is torn apart and
// its bins lose the phase relation that makes them one windowed sinusoid.  Here (Laroche & Dolson 1999, identity locking with integer
// offsets; the definition is tests/pv_lock_reference.py) the frame's spectral peaks are found, every bin belongs to its nearest peak, and
// a peak's whole region is translated by ONE integer offset floor(P r + 0.5) - P and rotated by ONE angle, the peak's accumulated
// theta[P] + nu[P] (r - 1) / O, wrapped every frame.  The synthesis is a gather with one source per bin; the angle of a region is handed to
// all of its bins, so that a peak that moves to a neighbouring bin continues the angle of the region it was in.
//
// vp_k_stft_pv_lock and vp_k_pv_stream_lock are WRITTEN-OUT COPIES of vp_k_stft_pv_curve and vp_k_pv_stream_curve (docs/HISTORY.md, "One
// phase-vocoder stage for both kernels", for why copies): framing, transforms, ratio table, overlap-add, state record and bookkeeping are
// the parents', statement for statement.  The stage between split and merge is replaced; what differs is marked "lock:".
//
// State: theta lives where the parents keep the synthesis accumulator (PvLds::sum, the record's second array) and the previous frame's
// phases where they keep them (phPrev), so plain, curve, formant and locked calls may follow each other on one streaming handle; after a
// change of kind the output is defined and finite but carries a phase jump.
//
// lock: LDS on top of the parents' carve, per wavefront: the two 513-bit masks (peaks, shifted peaks) as nine 64-bit words each, the owner
// of every bin and the map from a shifted peak back to its peak.  The wavefront's `ana` row holds the complex spectrum (not magnitude and
// frequency), its `inc` row the magnitudes and then, at peaks, the angle's advance.
#define PV_LOCK_WORDS 10                                                       // nine used; ten keeps the int arrays 16-byte aligned
#define PV_LOCK_INTS 520                                                       // 513 used
#define PV_LOCK_WV_BYTES (2 * PV_LOCK_WORDS * 8 + 2 * PV_LOCK_INTS * 4)
__host__ __device__ constexpr size_t pv_lock_lds_bytes() { return (size_t)NWV * PV_LOCK_WV_BYTES; }

typedef __attribute__((address_space(3))) unsigned long long lds_u64;
typedef __attribute__((address_space(3))) int lds_i32;

struct PvLockLds {
    lds_u64 *peaks;            // [9] bit k & 63 of word k >> 6: bin k is a peak of this wavefront's frame
    lds_u64 *moved;            // [9] ... is a shifted peak P'
    lds_i32 *own;              // [513] the peak that owns bin k
    lds_i32 *back;             // [513] P' -> P, -1 elsewhere
};
__device__ __forceinline__ PvLockLds pv_lock_carve(lds_f64 *p, int wv)
{
    PvLockLds l;
    lds_u64 *w = (lds_u64 *)p + (size_t)wv * (PV_LOCK_WV_BYTES / 8);
    l.peaks = w; l.moved = w + PV_LOCK_WORDS;
    l.own = (lds_i32 *)(w + 2 * PV_LOCK_WORDS); l.back = l.own + PV_LOCK_INTS;
    return l;
}

// bin e of the lane's nine: even e the pair's k = 64 (e / 2) + lane, odd e its mirror 512 - k, e = 8 bin 256 (lane 0 only)
__device__ __forceinline__ int pv_lock_bin(int e, int lane) { return e == 8 ? 256 : (e & 1) ? 512 - (64 * (e >> 1) + lane) : 64 * (e >> 1) + lane; }

// The 513-bit mask of a per-bin flag from its nine ballots (bal[e]: bit `lane` is the flag of bin pv_lock_bin(e, lane)), written by lane 0.
// The pairs' words are the ballots; a mirror ballot reversed and moved up by one is bins 512 - 64 q - lane, lane = 1 .. 63, of word 7 - q,
// and its lane 0 is bit 0 of word 8 - q.
__device__ __forceinline__ void pv_lock_mask(lds_u64 *W, const unsigned long long (&bal)[9], bool lane0)
{
    if (!lane0) return;
#pragma unroll
    for (int q = 0; q < 4; q++) W[q] = bal[2 * q];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const unsigned long long below = q < 3 ? bal[2 * q + 3] : bal[8];      // bin 64 (7 - q): lane 0 of the next mirror, or bin 256
        W[7 - q] = (__builtin_bitreverse64(bal[2 * q + 1]) << 1) | (below & 1ull);
    }
    W[8] = bal[1] & 1ull;
}

// the set bit of the mask nearest to bin k (0 .. 512), the lower one on equal distance; -1 if the mask is empty
__device__ __forceinline__ int pv_lock_nearest(const lds_u64 *W, int k)
{
    const int wi = k >> 6, b = k & 63;
    const unsigned long long w0 = W[wi];
    unsigned long long x = w0 & (~0ull >> (63 - b));                           // bits 0 .. b
    int j = wi;
    while (x == 0ull && j > 0) x = W[--j];
    const int lo = x ? 64 * j + 63 - __builtin_clzll(x) : -1;
    x = b == 63 ? 0ull : w0 & (~0ull << (b + 1));                              // bits b + 1 .. 63
    j = wi;
    while (x == 0ull && j < 8) x = W[++j];
    const int hi = x ? 64 * j + __builtin_ctzll(x) : -1;
    if (lo < 0) return hi;
    if (hi < 0) return lo;
    return (k - lo <= hi - k) ? lo : hi;
}

// lock: everything of the stage in front of the turns, by one live wavefront: magnitudes, phases and the spectrum to LDS are the caller's
// (before its barrier); here peaks, owners, the peaks' advance of the angle (into the wavefront's `inc` row), the shifted peaks and the
// gather's indices.  own[e]: the peak that owns the lane's bin e; src[e]: the source bin of synthesis bin e or -1 (zero); pk[e]: the peak
// whose angle rotates it.  Returns whether the frame has a peak (wavefront-uniform).
__device__ __forceinline__ bool pv_lock_plan(const PvLds &pv, const PvLockLds &lk, int wv, int prevSlot, int ln, bool lane0, double ratio, double invO, int O,
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
            const int pa = lk.back[ps];
            const int k = kk - (ps - pa);
            pk[e] = pa;
            src[e] = (k >= 0 && k <= N && lk.own[min(max(k, 0), N)] == pa) ? k : -1;
        }
    }
    return true;
}

// lock: a wavefront's turn at theta (pv.sum), in frame order between the caller's barriers: every bin takes its owner's new angle; then
// the angles that rotate the lane's synthesis bins are read back (theta[P] of a peak is its own new angle).
__device__ __forceinline__ void pv_lock_turn(const PvLds &pv, int wv, int ln, bool lane0, const int (&own)[9], const int (&src)[9], const int (&pk)[9], double (&th)[9])
{
    constexpr int nb = 513;
    double t[9];
#pragma unroll
    for (int e = 0; e < 9; e++) {
        t[e] = pv.sum[own[e]] + pv.inc[wv * nb + own[e]];
        t[e] -= rint(t[e]);
    }
    wave_sync();                                                               // (other lanes read theta[P] of bins this lane overwrites)
#pragma unroll
    for (int e = 0; e < 9; e++) if (e < 8 || lane0) pv.sum[pv_lock_bin(e, ln)] = t[e];
    wave_sync();
#pragma unroll
    for (int e = 0; e < 9; e++) th[e] = src[e] >= 0 ? pv.sum[pk[e]] : 0.0;
}

// lock: the gather: synthesis bin e of the lane is its source bin of the wavefront's spectrum rotated by th[e], or zero
__device__ __forceinline__ void pv_lock_gather(const PvLds &pv, bool lane0, const int (&src)[9], const double (&th)[9], RPairs &X)
{
#pragma unroll
    for (int e = 0; e < 9; e++) {
        if (e == 8 && !lane0) continue;
        double re = 0.0, im = 0.0;
        if (src[e] >= 0) {
            const d2 x = pv.ana[src[e]];
            double sn, cs;
            pv_sincos_turns(th[e], sn, cs);
            re = __builtin_fma(x.x, cs, -(x.y * sn));
            im = __builtin_fma(x.x, sn, x.y * cs);
        }
        if (e == 8) { X.hr = re; X.hi = im; }
        else if (e & 1) { X.mr[e >> 1] = re; X.mi[e >> 1] = im; }
        else { X.kr[e >> 1] = re; X.ki[e >> 1] = im; }
    }
    if (lane0) { X.ki[0] = 0.0; X.mi[0] = 0.0; }
}

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv_lock(VpStftArgs A, const double *ratioTab)
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
    const PvLockLds lk = pv_lock_carve((lds_f64 *)smem + (stft_lds_base(F, hop) + pv_lds_bytes()) / 8, wv);   // lock:
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
            // ---- lock: the peak-locked stage, phases in TURNS (to the merge)
            const int nb = N + 1;
            const double invO = 1.0 / (double)O;
            // lock: (the lane number through a register the compiler cannot see through: vp_k_stft_pv2k)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            if (live) {
                // lock: spectrum, magnitude and phase of the lane's bins, straight to LDS
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
            if (live) has = pv_lock_plan(pv, lk, wv, wv, ln, lane0, ratio, invO, O, own, src, pk);
            // lock: theta is handed through the round in frame order, in place
            double th[9];
#pragma unroll
            for (int e = 0; e < 9; e++) th[e] = 0.0;
#pragma unroll
            for (int w = 0; w < NWV; w++) {
                if (w > 0) __syncthreads();
                if (live && has && wv == w) pv_lock_turn(pv, wv, ln, lane0, own, src, pk, th);
            }
            if (live) pv_lock_gather(pv, lane0, src, th, X);
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
            // ---- lock: end of the stage
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

// ---- streaming: vp_k_pv_stream_curve with the locked stage.  theta is the record's second array, handed from the call's first live frame
// to its last whatever their wavefronts.  The call's bookkeeping is written out, as in vp_k_pv_stream_curve (the comment there says why).
__global__ __launch_bounds__(64 * NWV) void vp_k_pv_stream_lock(VpPvArgs A, const double *ratioTab)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x;
    constexpr int N = 512, F = 1024, nb = N + 1, RM = VP_PV_RING - 1;
    const int hop = A.hop, O = A.O, L = A.L, NB = A.N, S = A.S;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *ring = (lds_f32 *)smem + NWV * 2048;                              // [VP_PV_RING]
    lds_f32 *hist = ring + VP_PV_RING;                                         // [F]
    const PvLds pv = pv_lds_carve((lds_f64 *)(hist + F), wv);
    const PvLockLds lk = pv_lock_carve((lds_f64 *)smem + pv_stream_lds_bytes() / 8, wv);   // lock:
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

    const int M = A.nBlocks * NB;
    const long long R = n + M;
    const long long fa = n >= F ? (n - F) / hop + 1 : 0;
    const long long fb = R >= F ? (R - F) / hop + 1 : 0;
    const int nf = (int)(fb - fa);
    const int H = (int)(n - fa * hop);
    const int er = H - L;
    const int fr0 = -(int)(fa & 3);

    for (int i = tid; i < H; i += 64 * NWV) hist[i] = recHist[i];
    for (int i = tid; i < nb; i += 64 * NWV) { pv.phPrev[i] = rst ? 0.0 : recD[i]; pv.sum[i] = rst ? 0.0 : recD[nb + i]; }
    for (int q = tid; q < VP_PV_RING; q += 64 * NWV) {
        const int i = (q - er) & RM;
        ring[q] = (i < F && !rst) ? recCarry[i] : 0.f;
    }

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
    auto sample = [&](int rel) -> float {
        if (rel < H) return hist[rel];
        const unsigned c = (unsigned)(rel - H), b = c / (unsigned)NB;
        return xs[(size_t)b * S * NB + (c - b * NB)];
    };
    auto emit = [&](int c, float v) {
        const unsigned b = (unsigned)c / (unsigned)NB;
        ys[(size_t)b * S * NB + ((unsigned)c - b * NB)] = v;
    };
    const int nRounds = nf > 0 ? (nf - fr0 + NWV - 1) / NWV : 0;
    int cb = er;
    f2 xv[8];
    double rq = 1.0;
    auto request = [&](int k_) {
        const int fr_ = fr0 + NWV * k_ + wv;
        if (k_ < nRounds && fr_ >= 0 && fr_ < nf) {
#pragma unroll
            for (int r = 0; r < 8; r++) { const int rel = fr_ * hop + 2 * (lane + 64 * r); xv[r] = f2{sample(rel), sample(rel + 1)}; }
            const unsigned blk = (unsigned)(fr_ * hop + F - 1 - H) / (unsigned)NB;   // the block in which the frame's last sample arrives
            rq = ratioTab[(size_t)blk * S + s];
        }
    };
    request(0);
    for (int k = 0; k < nRounds; k++) {
        const int frW0 = fr0 + NWV * k;
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
            // ---- lock: the peak-locked stage (vp_k_stft_pv_lock's), to the merge
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
            if (live) has = pv_lock_plan(pv, lk, wv, prevSlot, ln, lane0, ratio, invO, O, own, src, pk);
            // lock: theta continues from the state at the call's first live frame and is left by its last
            double th[9];
#pragma unroll
            for (int e = 0; e < 9; e++) th[e] = 0.0;
#pragma unroll
            for (int w = 0; w < NWV; w++) {
                if (w > 0) __syncthreads();
                if (live && has && wv == w) pv_lock_turn(pv, wv, ln, lane0, own, src, pk, th);
            }
            if (live) pv_lock_gather(pv, lane0, src, th, X);
            if (live && wv == wLast) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k_ = pv_lock_bin(e, ln);
                    pv.phPrev[k_] = pv.phPrev[(wv + 1) * nb + k_];
                }
            }
            // ---- lock: end of the stage
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
        const int frA = frW0 + wFirst, frB = frW0 + wLast;
        const int lo = frA * hop, hi = frB * hop + F;
        for (int j = lo + ((tid - lo) & (64 * NWV - 1)); j < hi; j += 64 * NWV) {
            float v = ring[j & RM];
            for (int w = wFirst; w <= wLast; w++) {
                const int o = j - (frW0 + w) * hop;
                if (o >= 0 && o < F) v += slots[w * 2048 + o];
            }
            ring[j & RM] = v;
        }
        const int emitEnd = min((frB + 1) * hop, er + M);
        for (int j = cb + ((tid - cb) & (64 * NWV - 1)); j < emitEnd; j += 64 * NWV) { emit(j - er, ring[j & RM]); ring[j & RM] = 0.f; }
        cb = max(cb, emitEnd);
        __syncthreads();
    }
    for (int j = cb + ((tid - cb) & (64 * NWV - 1)); j < er + M; j += 64 * NWV) { emit(j - er, ring[j & RM]); ring[j & RM] = 0.f; }

    const int Hn = H + M - nf * hop;
    for (int i = tid; i < Hn; i += 64 * NWV) recHist[i] = sample(nf * hop + i);
    const int ern = er + M;
    for (int q = tid; q < VP_PV_RING; q += 64 * NWV) {
        const int i = (q - ern) & RM;
        if (i < F) recCarry[i] = ring[q];
    }
    __syncthreads();
    for (int i = tid; i < nb; i += 64 * NWV) { recD[i] = pv.phPrev[i]; recD[nb + i] = pv.sum[i]; }
    if (tid == 0) { recD[VP_PV_RATIO] = recRatio; ((long long *)recD)[VP_PV_COUNT] = R; }
}

hipError_t vp_stft_lock_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_stft_pv_lock, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

size_t vp_stft_lock_lds_bytes(int hop) { return stft_lds_base(1024, hop) + pv_lds_bytes() + pv_lock_lds_bytes(); }
size_t vp_pv_lock_lds_bytes() { return pv_stream_lds_bytes() + pv_lock_lds_bytes(); }

hipError_t vp_stft_launch_lock(const VpStftArgs &a, const double *d_ratio, int nStreams, hipStream_t st)
{
    const dim3 grid(1, nStreams), block(64 * NWV);                             // (one run: theta is a recurrence over the stream's frames)
    hipLaunchKernelGGL(vp_k_stft_pv_lock, grid, block, vp_stft_lock_lds_bytes(a.hop), st, a, d_ratio);
    return hipGetLastError();
}

hipError_t vp_pv_lock_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_pv_stream_lock, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_pv_launch_lock(const VpPvArgs &a, const double *d_ratio, hipStream_t st)
{
    hipLaunchKernelGGL(vp_k_pv_stream_lock, dim3(a.S), dim3(64 * NWV), vp_pv_lock_lds_bytes(), st, a, d_ratio);
    return hipGetLastError();
}
