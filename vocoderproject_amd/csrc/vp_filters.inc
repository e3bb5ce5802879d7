// vp_filters.inc -- part of vp_kernels.hip (included there; not a translation unit of its own):
// wave-level building blocks shared by the vocoder and pitch kernels: Levinson-Durbin forms, autocorrelation stretches,
// residual FIRs, energies, and every form of the all-pole recursion (exact, FAST, block forms).

// ------------------------------------------------------------------------------------------------
// Wave-uniform broadcast of a double held by lane `src` (src is wave-uniform): two v_readlane_b32.
__device__ __forceinline__ double bcast_f64(double v, int src)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, src);
    hi = __builtin_amdgcn_readlane(hi, src);
    return __hiloint2double(hi, lo);
}

// Levinson-Durbin (LPC.cpp:107-148) by ONE WAVEFRONT with the coefficient vector spread over the
// lanes: lane l owns a[l] and a[64+l].  The two dot products of every order step are summed in the
// reference's order (i = 1..p-1, left to right) by broadcasting the per-lane products one after
// the other, so the result is bit-identical to the serial recursion; the products and the
// coefficient update run lane-parallel.  All 64 lanes must call it (wave-uniform arguments).
// `scratch` (LDS, 16-byte aligned, >= 128 doubles) lets orders below 64 take a cheaper route for the
// ordered sums: the lanes park their two products side by side in LDS and every lane then reads
// them back in order, four steps per trip, instead of 4 v_readlane per step.
template <class RP, class AP>
__device__ __forceinline__ bool levinson_wave(RP r, AP a, int order, int aLen, double eps, lds_f64 *scratch = nullptr)
{
    const int lane = vp_tid() & 63;
    if (fabs(r[0]) < eps) {                        // :110-114 (floating abs intended, SURVEY.md Q1)
        for (int i = lane; i < aLen; i += WAVE) a[i] = (i == 0) ? 1.0 : 0.0;
        return true;                               // the whole vector was rewritten
    }
    const double r0 = r[0];
    if (scratch && order < WAVE) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        typedef __attribute__((address_space(3))) d2 lds_d2;
        lds_d2 *pr = (lds_d2 *)scratch;                 // pr[i] = { r[p-i]*a[i], r[i]*a[i] }
        double av = 0.0;                                 // a[lane]
        if (lane == 0) av = 1.0;
        if (lane == 1) av = r[1] / r0;
        const double rl = (lane <= order) ? r[lane] : 0.0;
        for (int p = 2; p < order + 1; p++) {
            const bool in = lane >= 1 && lane < p;
            d2 qs;
            qs.x = in ? r[p - lane] * av : 0.0;
            qs.y = rl * av;
            pr[lane] = qs;
            double rho_a = 0.0, r_a = 0.0;
            int i = 1;
            for (; i + 4 <= p; i += 4) {                 // i .. i+3 < p
                const d2 v0 = pr[i], v1 = pr[i + 1], v2 = pr[i + 2], v3 = pr[i + 3];
                rho_a += v0.x; r_a += v0.y;
                rho_a += v1.x; r_a += v1.y;
                rho_a += v2.x; r_a += v2.y;
                rho_a += v3.x; r_a += v3.y;
            }
            for (; i < p; i++) { const d2 v = pr[i]; rho_a += v.x; r_a += v.y; }
            const double k = (r[p] - rho_a) / (r0 - r_a);
            const double partner = __shfl(av, (p - lane) & 63, WAVE);     // aPrev[p - i]
            double nv = av;
            if (in) nv = av - k * partner;
            if (lane == p) nv = k;
            av = nv;
        }
        if (lane >= 1) av *= -1.;
        if (lane <= order) a[lane] = av;
        return false;
    }
    double a0 = 0.0, a1 = 0.0;                      // a[lane], a[64+lane]
    if (lane == 0) a0 = 1.0;
    if (lane == 1) a0 = r[1] / r0;
    const double rl0 = (lane <= order) ? r[lane] : 0.0;             // r[i] for i = lane
    const double rl1 = (64 + lane <= order) ? r[64 + lane] : 0.0;   // r[i] for i = 64+lane
    for (int p = 2; p < order + 1; p++) {
        // per-lane products for i = lane and i = 64+lane (only 1 <= i < p are consumed)
        const int i0 = lane, i1 = 64 + lane;
        double q0 = (i0 >= 1 && i0 < p) ? r[p - i0] * a0 : 0.0;
        double q1 = (i1 < p) ? r[p - i1] * a1 : 0.0;
        double s0 = rl0 * a0, s1 = rl1 * a1;
        double rho_a = 0.0, r_a = 0.0;
        const int n0 = min(p, 64);
        for (int i = 1; i < n0; i++) { rho_a += bcast_f64(q0, i); r_a += bcast_f64(s0, i); }
        for (int i = 64; i < p; i++) { rho_a += bcast_f64(q1, i - 64); r_a += bcast_f64(s1, i - 64); }
        const double k = (r[p] - rho_a) / (r0 - r_a);
        // a[i] = aPrev[i] - k * aPrev[p - i], 1 <= i < p
        int j0 = p - i0, j1 = p - i1;                               // partner indices
        double p0lo = __shfl(a0, j0 & 63, WAVE), p0hi = __shfl(a1, j0 & 63, WAVE);
        double p1lo = __shfl(a0, j1 & 63, WAVE), p1hi = __shfl(a1, j1 & 63, WAVE);
        double n0v = a0, n1v = a1;
        if (i0 >= 1 && i0 < p) n0v = a0 - k * ((j0 >= 64) ? p0hi : p0lo);
        if (i1 < p) n1v = a1 - k * ((j1 >= 64) ? p1hi : p1lo);
        if (i0 == p) n0v = k;
        if (i1 == p) n1v = k;
        a0 = n0v; a1 = n1v;
    }
    if (lane >= 1) a0 *= -1.;                       // :145-146 (entries beyond the order are 0 -> -0, never read)
    a1 *= -1.;
    if (lane <= order) a[lane] = a0;
    if (64 + lane <= order) a[64 + lane] = a1;
    return false;
}

// RUN += (lane U of V's 16-lane row) * ONE in one VALU op (DPP row broadcast; ONE must hold 1.0, so the
// fused multiply-add rounds exactly like RUN + value).
#define VP_FMAC_BCAST(RUN, V, ONE, U) \
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #U " row_mask:0xf bank_mask:0xf" : "+v"(RUN) : "v"(V), "v"(ONE))

// A stretch [n0, n1) of the LPC autocorrelation sum_n x[n] x[n+m] (LPC.cpp:44-97), continued from `sum`,
// by one full wavefront with lane -> lag m.  n0 and n1 are multiples of 8 and n1 <= F - (largest lag).
// Eight elements per trip, the next trip's LDS reads issued before this trip's arithmetic; product and
// sum stay two roundings, in the reference's order.  (v_mul_f64 has no DPP form on gfx950 -- only
// v_fmac_f64 does -- so the wave-uniform factor x[n] is an LDS broadcast read.)
__device__ __forceinline__ double autocorr_stretch(const lds_f64 *x, int m, int n0, int n1, double sum)
{
    const lds_f64 *xm = x + m;
    if (n0 >= n1) return sum;
    double a0[8], b0[8], a1[8], b1[8];
#define VP_ALOAD(A, B, I) _Pragma("unroll") for (int u = 0; u < 8; u++) { A[u] = x[(I) + u]; B[u] = xm[(I) + u]; }
#define VP_ACOMP(A, B) { double p_[8]; _Pragma("unroll") for (int u = 0; u < 8; u++) p_[u] = A[u] * B[u]; \
                         __builtin_amdgcn_sched_barrier(0); \
                         _Pragma("unroll") for (int u = 0; u < 8; u++) sum += p_[u]; \
                         __builtin_amdgcn_sched_barrier(0); }
    VP_ALOAD(a0, b0, n0)
    for (int n = n0; n < n1; n += 16) {
        const bool more1 = n + 8 < n1;
        if (more1) { VP_ALOAD(a1, b1, n + 8) }
        VP_ACOMP(a0, b0)
        if (more1) {
            if (n + 16 < n1) { VP_ALOAD(a0, b0, n + 16) }
            VP_ACOMP(a1, b1)
        }
    }
#undef VP_ALOAD
#undef VP_ACOMP
    return sum;
}

// The LPC autocorrelation (LPC.cpp:44-97) in the reference's own arithmetic -- every lag one left-to-right sum of rounded
// products -- with the PRODUCTS lane-parallel and only the sums serial (round 3; bit-identical to autocorr_stretch).  Lane
// (row, m) of the calling wavefront forms x[n0 + m] * x[n0 + m + lag] for sixteen consecutive n at once (one v_mul_f64 per
// chain), lag = lag0 + row for chain A and lag0 + 4 + row for chain B; the ordered sums are then chains of v_fmac_f64 with a
// DPP row-broadcast operand, sum += product(lane u) * 1.0 for u = 0..15 -- x * 1.0 + s rounds exactly like s + x, and a
// product masked to +0.0 past the frame's end adds nothing --, the two chains interleaved.  Eight lags per wavefront and pass,
// 34 vector instructions and three LDS reads per sixteen elements; the lane-per-lag form spends 32 LDS reads on the same
// sixteen elements and keeps 16 of 64 lanes busy (25 us per 1024-sample frame at order 15; this: 7.4 us on each of two
// wavefronts).  Pays for order + 1 <= 32 lags (each pass covers eight; the lane-per-lag form covers 64 in one).
// r: LDS vector [order + 1].  All 64 lanes must call it.
template <class RP>
__device__ __forceinline__ void autocorr_rows_exact8(const lds_f64 *x, int F, int order, int lag0, RP r)
{
    const int lane = vp_tid() & 63, m = lane & 15, row = lane >> 4;
    const int lagA = lag0 + row, lagB = lag0 + 4 + row;
    const lds_f64 *xm = x + m, *xa = xm + lagA, *xb = xm + lagB;
    const double one = vp_one();
    double sA = 0.0, sB = 0.0;
    const int nFull = max(0, F - 15 - (lag0 + 7));                            // trips that start below it lie inside the sums of all eight lags
#define VP_ACE_CHAIN \
        asm volatile("s_nop 1" : "+v"(pA), "+v"(pB));                         /* VALU write -> DPP read */ \
        VP_FMAC_BCAST(sA, pA, one, 0);  VP_FMAC_BCAST(sB, pB, one, 0);  VP_FMAC_BCAST(sA, pA, one, 1);  VP_FMAC_BCAST(sB, pB, one, 1); \
        VP_FMAC_BCAST(sA, pA, one, 2);  VP_FMAC_BCAST(sB, pB, one, 2);  VP_FMAC_BCAST(sA, pA, one, 3);  VP_FMAC_BCAST(sB, pB, one, 3); \
        VP_FMAC_BCAST(sA, pA, one, 4);  VP_FMAC_BCAST(sB, pB, one, 4);  VP_FMAC_BCAST(sA, pA, one, 5);  VP_FMAC_BCAST(sB, pB, one, 5); \
        VP_FMAC_BCAST(sA, pA, one, 6);  VP_FMAC_BCAST(sB, pB, one, 6);  VP_FMAC_BCAST(sA, pA, one, 7);  VP_FMAC_BCAST(sB, pB, one, 7); \
        VP_FMAC_BCAST(sA, pA, one, 8);  VP_FMAC_BCAST(sB, pB, one, 8);  VP_FMAC_BCAST(sA, pA, one, 9);  VP_FMAC_BCAST(sB, pB, one, 9); \
        VP_FMAC_BCAST(sA, pA, one, 10); VP_FMAC_BCAST(sB, pB, one, 10); VP_FMAC_BCAST(sA, pA, one, 11); VP_FMAC_BCAST(sB, pB, one, 11); \
        VP_FMAC_BCAST(sA, pA, one, 12); VP_FMAC_BCAST(sB, pB, one, 12); VP_FMAC_BCAST(sA, pA, one, 13); VP_FMAC_BCAST(sB, pB, one, 13); \
        VP_FMAC_BCAST(sA, pA, one, 14); VP_FMAC_BCAST(sB, pB, one, 14); VP_FMAC_BCAST(sA, pA, one, 15); VP_FMAC_BCAST(sB, pB, one, 15);
    int n0 = 0;
    double xv = xm[0], ya = xa[0], yb = xb[0];
    for (; n0 < nFull; n0 += 16) {
        double pA = xv * ya, pB = xv * yb;
        xv = xm[n0 + 16]; ya = xa[n0 + 16]; yb = xb[n0 + 16];                 // the next trip's operands (possibly past the frame: masked below, or unused)
        VP_ACE_CHAIN
    }
    for (; n0 < F; n0 += 16) {                                                // the sums' ends: a product exists for n + lag < F
        double pA = (n0 + m + lagA < F) ? xv * ya : 0.0, pB = (n0 + m + lagB < F) ? xv * yb : 0.0;
        xv = xm[n0 + 16]; ya = xa[n0 + 16]; yb = xb[n0 + 16];
        VP_ACE_CHAIN
    }
#undef VP_ACE_CHAIN
    if (m == 0) {
        if (lagA <= order) r[lagA] = sA / vp_f64_here(F);
        if (lagB <= order) r[lagB] = sB / vp_f64_here(F);
    }
}

// FAST mode (VP_IIR_FAST, the tolerance mode): the LPC autocorrelation r[m] = (1/F) sum_{n < F-m} x[n] x[n+m] (LPC.cpp:44-97)
// with the sum over n SPLIT across the wavefront instead of one left-to-right chain per lag: lane (s = lane >> 4,
// m = lane & 15) sums lag 16 grp + m over the s-th quarter of the frame as a chain of fused multiply-adds -- the
// quarter's x[n] reach the row through the DPP row broadcast (one LDS read per sixteen elements), the lane's own
// x[n + lag] slide through registers -- and the four quarters meet in a two-level shuffle tree.  All 64 lanes work (the
// ordered form keeps order + 1 of them busy for F dependent adds: 25 us per frame at order 15 against 2 here).  Not the
// reference's summation order: r[] differs at the 1e-16 relative level; nothing discrete depends on it (the marks and
// YIN read the raw voice), so this is tolerance-mode arithmetic exactly like the FAST recursions.
// Called by full wavefronts; the caller takes the groups of sixteen lags grp0, grp0 + grpStep, ... (orders above 15: several
// groups, which two wavefronts can share); r: LDS vector [order + 1].
#define VP_ACR_T2(XX, OWN, U, ACC) VP_FMAC_BCAST(ACC, XX, OWN[U], U);
#define VP_ACR_TRIP2(XX, OWN, A0, A1) VP_ACR_T2(XX, OWN, 0, A0) VP_ACR_T2(XX, OWN, 1, A1) VP_ACR_T2(XX, OWN, 2, A0) VP_ACR_T2(XX, OWN, 3, A1) \
    VP_ACR_T2(XX, OWN, 4, A0) VP_ACR_T2(XX, OWN, 5, A1) VP_ACR_T2(XX, OWN, 6, A0) VP_ACR_T2(XX, OWN, 7, A1) VP_ACR_T2(XX, OWN, 8, A0) \
    VP_ACR_T2(XX, OWN, 9, A1) VP_ACR_T2(XX, OWN, 10, A0) VP_ACR_T2(XX, OWN, 11, A1) VP_ACR_T2(XX, OWN, 12, A0) VP_ACR_T2(XX, OWN, 13, A1) \
    VP_ACR_T2(XX, OWN, 14, A0) VP_ACR_T2(XX, OWN, 15, A1)

// one group of sixteen lags from trip i on (acc0/acc1: what the caller has summed of it so far): the unconditional trips up to the
// group's own limit, the masked trips of the frame's end, the shuffle tree, the store
template <bool AHEAD, class RP>
__device__ __forceinline__ void autocorr_rows_fast_group(const lds_f64 *x, int F, int order, RP r, int grp, int i, double acc0, double acc1)
{
    const int lane = vp_tid() & 63, m = lane & 15, s = lane >> 4;
    const int seg = ((F + 63) >> 6) << 4;                                     // quarter length, a multiple of 16
    const int n0 = s * seg;
    const int lag = 16 * grp + m;
    const int lim = F - lag;                                                  // products exist for n < lim
    const lds_f64 *xl = x + lag;
    // trips whose sixteen elements lie inside every lane's range take their operands unconditionally
    const int iEnd = min(max(0, (F - 3 * seg - 16 * grp - 15) & ~15), seg);
#define VP_ACR_LOAD(XX, OWN, I) { const int n_ = n0 + (I); XX = x[n_ + m]; _Pragma("unroll") for (int u = 0; u < 16; u++) OWN[u] = xl[n_ + u]; }
    if (AHEAD) {
        // two register sets: the next trip's seventeen operands are requested before this trip's arithmetic
        double Xa = 0.0, Xb = 0.0, oa[16], ob[16];
        const int iStart = i;
        if (i < iEnd) VP_ACR_LOAD(Xa, oa, i)
        for (; i < iEnd; i += 32) {
            const bool more = i + 16 < iEnd;
            if (more) VP_ACR_LOAD(Xb, ob, i + 16)
            VP_ACR_TRIP2(Xa, oa, acc0, acc1)
            if (more) {
                if (i + 32 < iEnd) VP_ACR_LOAD(Xa, oa, i + 32)
                VP_ACR_TRIP2(Xb, ob, acc0, acc1)
            }
        }
        i = max(iStart, iEnd);                                                // (the loop steps by 32: back to the first trip not done)
    } else
    for (; i < iEnd; i += 16) {
        double X, own[16];                                                    // x[n + u] sits in lane u of the row
        VP_ACR_LOAD(X, own, i)
        VP_ACR_TRIP2(X, own, acc0, acc1)
    }
#undef VP_ACR_LOAD
    for (; i < seg; i += 16) {                                                // the frame's end: operands past it count as zero
        const int n = n0 + i;
        double X = x[n + m];
        if (!(n + m < F)) X = 0.0;
        double own[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { const double v = xl[n + u]; own[u] = (n + u < lim) ? v : 0.0; }
        asm volatile("s_nop 1" : "+v"(X));                                    // VALU write -> DPP read
        VP_ACR_TRIP2(X, own, acc0, acc1)
    }
    double t = acc0 + acc1;
    t += __shfl_xor(t, 16, WAVE);
    t += __shfl_xor(t, 32, WAVE);
    if (lane < 16 && lag <= order) r[lag] = t / vp_f64_here(F);
}

// Lags 0..15 over HALF of the frame (round 4), so that two wavefronts can share the sums (the pitch kernel's YIN phase leaves wave 6
// idle: 4.1 us of the last wavefront's LPC chain become 2).  The half is dealt to the wavefront's four rows in INTERLEAVED trips of
// sixteen elements -- row s takes elements 64 t + 16 s .. + 15 of the half -- so that the two rows of a ds_read_b64 lane group read 32
// consecutive doubles, all 64 banks once (rows a whole quarter apart, as in autocorr_rows_fast_group, sit 128 doubles = 0 banks apart:
// a 2-way conflict on all seventeen reads of a trip).  Returns, in lanes 0..15, the half's sum for lag = lane (not yet divided by F);
// r[lag] = (half 0 + half 1) / F whoever computes the halves -- one wavefront both or two wavefronts one each -- so every build that
// uses this form gets the same bits.
template <bool AHEAD>
__device__ __forceinline__ double autocorr_rows_fast_half(const lds_f64 *x, int F, int half)
{
    const int lane = vp_tid() & 63, m = lane & 15, s = lane >> 4;
    const int hl = ((F + 127) >> 7) << 6;                                     // half length, a multiple of 64
    const int n0 = half * hl + 16 * s;                                        // the row's first element; its trips are 64 apart
    const int lim = F - m;                                                    // products exist for n < lim
    const lds_f64 *xl = x + m;
    const int nT = hl >> 6;                                                   // trips per row
    // trips whose sixteen elements (and the fifteen lags behind them) lie inside the frame for EVERY row take their operands unconditionally
    const int tEnd = min(max(0, (F - half * hl - 48 - 30 + 63) >> 6), nT);
    double acc0 = 0.0, acc1 = 0.0;
    int t = 0;
#define VP_ACR_LOAD(XX, OWN, T_) { const int n_ = n0 + 64 * (T_); XX = x[n_ + m]; _Pragma("unroll") for (int u = 0; u < 16; u++) OWN[u] = xl[n_ + u]; }
    if (AHEAD) {
        double Xa = 0.0, Xb = 0.0, oa[16], ob[16];
        if (t < tEnd) VP_ACR_LOAD(Xa, oa, t)
        for (; t < tEnd; t += 2) {
            const bool more = t + 1 < tEnd;
            if (more) VP_ACR_LOAD(Xb, ob, t + 1)
            VP_ACR_TRIP2(Xa, oa, acc0, acc1)
            if (more) {
                if (t + 2 < tEnd) VP_ACR_LOAD(Xa, oa, t + 2)
                VP_ACR_TRIP2(Xb, ob, acc0, acc1)
            }
        }
        t = tEnd;
    } else
    for (; t < tEnd; t++) {
        double X, own[16];
        VP_ACR_LOAD(X, own, t)
        VP_ACR_TRIP2(X, own, acc0, acc1)
    }
#undef VP_ACR_LOAD
    for (; t < nT; t++) {                                                     // the frame's end: operands past it count as zero
        const int n = n0 + 64 * t;
        double X = (n + m < F) ? x[min(n + m, F - 1)] : 0.0;
        double own[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { const double v = xl[max(0, min(n + u, lim - 1))]; own[u] = (n + u < lim) ? v : 0.0; }
        asm volatile("s_nop 1" : "+v"(X));                                    // VALU write -> DPP read
        VP_ACR_TRIP2(X, own, acc0, acc1)
    }
    double tt = acc0 + acc1;
    tt += __shfl_xor(tt, 16, WAVE);
    tt += __shfl_xor(tt, 32, WAVE);
    return tt;
}

// THREE groups (lags 16 g0 .. 16 g0 + 47) in one pass: group j's sixteen operands of trip i + 16 are group j + 1's of trip i, so
// a trip loads sixteen new values (the top group's) and reuses thirty-two -- 17 LDS reads for 48 multiply-adds instead of 51 --
// with FOUR register sets rotating by name (the fourth receives the next trip's load during this trip's arithmetic).  Per lane
// the same products are added in the same order as by three single-group passes: bit-identical to them.  A lone wavefront spends
// 16.7 us on the 49 lags of a 2048-sample frame group by group (each trip is bound by its LDS reads), 7 this way.
template <class RP>
__device__ __forceinline__ void autocorr_rows_fast3(const lds_f64 *x, int F, int order, RP r, int g0)
{
    const int lane = vp_tid() & 63, m = lane & 15, s = lane >> 4;
    const int seg = ((F + 63) >> 6) << 4;
    const int n0 = s * seg;
    const lds_f64 *xa = x + n0 + m;                                           // xa[i]: the row's broadcast operand of trip i
    const lds_f64 *xw = x + n0 + 16 * g0 + m;                                 // xw[i + u + 16 j]: group j's operand u of trip i
    // the trips all three groups take unconditionally (the top group's limit)
    const int iF3 = min(max(0, (F - 3 * seg - 16 * (g0 + 2) - 15) & ~15), seg);
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0, a20 = 0.0, a21 = 0.0;
    double A[16], B[16], C[16], D[16], X = 0.0, Xn = 0.0;
#define VP_ACR_LD(W, OFF) _Pragma("unroll") for (int u = 0; u < 16; u++) W[u] = xw[(OFF) + u];
#define VP_ACR_TRIP3(W0, W1, W2, WN) { \
        if (i + 16 < iF3) { VP_ACR_LD(WN, i + 48) Xn = xa[i + 16]; }          /* the next trip's top window and broadcast operand */ \
        VP_ACR_TRIP2(X, W0, a00, a01) VP_ACR_TRIP2(X, W1, a10, a11) VP_ACR_TRIP2(X, W2, a20, a21) \
        X = Xn; i += 16; }
    int i = 0;
    if (iF3 > 0) { VP_ACR_LD(A, 0) VP_ACR_LD(B, 16) VP_ACR_LD(C, 32) X = xa[0]; }
    while (i < iF3) {
        VP_ACR_TRIP3(A, B, C, D)
        if (i >= iF3) break;
        VP_ACR_TRIP3(B, C, D, A)
        if (i >= iF3) break;
        VP_ACR_TRIP3(C, D, A, B)
        if (i >= iF3) break;
        VP_ACR_TRIP3(D, A, B, C)
    }
#undef VP_ACR_TRIP3
#undef VP_ACR_LD
    autocorr_rows_fast_group<false>(x, F, order, r, g0, i, a00, a01);
    autocorr_rows_fast_group<false>(x, F, order, r, g0 + 1, i, a10, a11);
    autocorr_rows_fast_group<false>(x, F, order, r, g0 + 2, i, a20, a21);
}

// Called by full wavefronts; the caller takes the groups of sixteen lags grp0, grp0 + grpStep, ... up to grpLast (orders above
// 15: several groups, which two wavefronts can share); FUSE: runs of three consecutive groups go through autocorr_rows_fast3.
// r: LDS vector [order + 1].
template <bool AHEAD, bool FUSE = false, class RP>
__device__ __forceinline__ void autocorr_rows_fast(const lds_f64 *x, int F, int order, RP r, int grp0 = 0, int grpStep = 1, int grpLast = 1 << 20)
{
    const int lane = vp_tid() & 63;
    for (int grp = grp0; 16 * grp <= order && grp <= grpLast; grp += grpStep) {
        if (16 * grp == order && grp > 0) {
            // a single lag is left (orders 16, 32, 48): a group's trip would spend 15 of 16 lanes on lags beyond the order -- the
            // whole wavefront shares the one sum instead (element n to lane n & 63, shuffle tree)
            const lds_f64 *xo = x + order;
            double acc = 0.0;
            for (int n = lane; n < F - order; n += WAVE) acc = __builtin_fma(x[n], xo[n], acc);
            for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
            if (lane == 0) r[order] = acc / vp_f64_here(F);
            break;
        }
        if (FUSE && grpStep == 1 && 16 * (grp + 2) < order && grp + 2 <= grpLast) {   // three groups with lags to store
            autocorr_rows_fast3(x, F, order, r, grp);
            grp += 2;
            continue;
        }
        autocorr_rows_fast_group<AHEAD>(x, F, order, r, grp, 0, 0.0, 0.0);
    }
}
#undef VP_ACR_TRIP2
#undef VP_ACR_T2

// Levinson-Durbin for orders below 16 with the coefficient vector inside ONE 16-lane row (lane m of
// every row owns a[m]; the four rows of the calling wavefront work redundantly).  The ordered sums
// rho_a = sum_{i=1..p-1} r[p-i] a[i] and r_a = sum r[i] a[i] (LPC.cpp:120-128) are chains of
// v_fmac_f64 with a DPP row-broadcast operand: entries i >= p hold +0.0, and adding +0.0 to a sum that
// started from +0.0 changes nothing, so all fifteen terms are always added and no lane ever talks to
// the LDS for them (the general form's park-and-read-back costs two LDS round trips per order step).
template <class RP, class AP>
__device__ __forceinline__ bool levinson_row16(RP r, AP a, int order, int aLen, double eps)
{
    const int lane = vp_tid() & 63, m = lane & 15;
    if (fabs(r[0]) < eps) {                        // :110-114
        for (int i = lane; i < aLen; i += WAVE) a[i] = (i == 0) ? 1.0 : 0.0;
        return true;
    }
    const double r0 = r[0], one = vp_one();
    double av = 0.0;                                 // a[m]
    if (m == 0) av = 1.0;
    if (m == 1) av = r[1] / r0;
    const double rl = (m >= 1 && m <= order) ? r[m] : 0.0;
    double rq = (m >= 1 && m < 2) ? r[2 - m] : 0.0;  // r[p - m] of the coming step
    for (int p = 2; p < order + 1; p++) {
        const bool in = m >= 1 && m < p;
        double q = in ? rq * av : 0.0;
        double sv = rl * av;
        const double rp = r[p];
        const double partner = __shfl(av, (lane & 48) | ((p - m) & 15), WAVE);      // a[p - m]
        if (p + 1 < order + 1) rq = (m >= 1 && m < p + 1) ? r[p + 1 - m] : 0.0;
        double rho_a = 0.0, r_a = 0.0;
        asm volatile("s_nop 1" : "+v"(q), "+v"(sv));                             // VALU write -> DPP read
#define VP_LV(U) VP_FMAC_BCAST(rho_a, q, one, U); VP_FMAC_BCAST(r_a, sv, one, U);
        VP_LV(1) VP_LV(2) VP_LV(3) VP_LV(4) VP_LV(5) VP_LV(6) VP_LV(7) VP_LV(8)
        VP_LV(9) VP_LV(10) VP_LV(11) VP_LV(12) VP_LV(13) VP_LV(14) VP_LV(15)
#undef VP_LV
        const double k = (rp - rho_a) / (r0 - r_a);
        double nv = av;
        if (in) nv = av - k * partner;
        if (m == p) nv = k;
        av = nv;
    }
    if (m >= 1) av *= -1.;
    if (lane <= order) a[lane] = av;
    return false;
}

// Levinson-Durbin for orders 16..48, the row form above with THREE coefficient registers per lane: slot s = 16 j + m (register j,
// lane m of every 16-lane row) holds a[s + 1]; the four rows of the calling wavefront work redundantly.  Per order step: six
// lane-parallel products, the two ordered sums as chains of DPP row-broadcast fmacs over the registers in use (entries
// beyond p - 1 hold +0.0: adding them changes nothing), the partner a[p - i] of every slot through three in-row shuffles
// (the partner's lane, (p - 2 - m) & 15, is the same for all three registers), one lane-parallel update.  Against the
// register-resident scalar form (every lane the whole recursion: 6 (p - 1) instructions per step) this issues
// 2 * 16 * ceil((p - 1) / 16) + ~40: a third of the instructions at order 48, and no LDS traffic inside the sums.
template <class RP, class AP>
__device__ __forceinline__ bool levinson_row48(RP r, AP a, int order_, int aLen, double eps)
{
    const int lane = vp_tid() & 63, m = lane & 15;
    const int order = __builtin_amdgcn_readfirstlane(order_);
    if (fabs(r[0]) < eps) {                        // :110-114
        for (int i = lane; i < aLen; i += WAVE) a[i] = (i == 0) ? 1.0 : 0.0;
        return true;
    }
    const double r0 = r[0], one = vp_one();
    const int i0 = m + 1, i1 = m + 17, i2 = m + 33;                           // the indices this lane's three slots stand for
    double A0 = 0.0, A1 = 0.0, A2 = 0.0;                                      // a[i0], a[i1], a[i2]
    if (m == 0) A0 = r[1] / r0;
    const double R0 = (i0 <= order) ? r[i0] : 0.0, R1 = (i1 <= order) ? r[i1] : 0.0, R2 = (i2 <= order) ? r[i2] : 0.0;
    // r[p - i] of the coming step (valid for 1 <= i <= p - 1)
    double Q0 = (i0 <= 1) ? r[2 - i0] : 0.0, Q1 = 0.0, Q2 = 0.0;
    for (int p = 2; p <= order; p++) {
        const bool in0 = i0 <= p - 1, in1 = i1 <= p - 1, in2 = i2 <= p - 1;
        double q0 = in0 ? Q0 * A0 : 0.0, q1 = in1 ? Q1 * A1 : 0.0, q2 = in2 ? Q2 * A2 : 0.0;
        double s0 = R0 * A0, s1 = R1 * A1, s2 = R2 * A2;                      // (a beyond p - 1 is +0.0)
        const double rp = r[p];
        // partner a[p - i]: slot p - 2 - s, i.e. lane (p - 2 - m) & 15 of register ((p - 2 - m) >> 4) - j
        const int pm = p - 2 - m, src = (lane & 48) | (pm & 15), c = pm >> 4;
        const double P0 = __shfl(A0, src, WAVE), P1 = __shfl(A1, src, WAVE), P2 = __shfl(A2, src, WAVE);
        if (p + 1 <= order) {
            Q0 = (i0 <= p) ? r[p + 1 - i0] : 0.0;
            Q1 = (i1 <= p) ? r[p + 1 - i1] : 0.0;
            Q2 = (i2 <= p) ? r[p + 1 - i2] : 0.0;
        }
        double rho_a = 0.0, r_a = 0.0;
        asm volatile("s_nop 1" : "+v"(q0), "+v"(s0), "+v"(q1), "+v"(s1), "+v"(q2), "+v"(s2));   // VALU write -> DPP read
#define VP_LV(QQ, SS, U) VP_FMAC_BCAST(rho_a, QQ, one, U); VP_FMAC_BCAST(r_a, SS, one, U);
#define VP_LVROW(QQ, SS) VP_LV(QQ, SS, 0) VP_LV(QQ, SS, 1) VP_LV(QQ, SS, 2) VP_LV(QQ, SS, 3) VP_LV(QQ, SS, 4) VP_LV(QQ, SS, 5) VP_LV(QQ, SS, 6) VP_LV(QQ, SS, 7) \
        VP_LV(QQ, SS, 8) VP_LV(QQ, SS, 9) VP_LV(QQ, SS, 10) VP_LV(QQ, SS, 11) VP_LV(QQ, SS, 12) VP_LV(QQ, SS, 13) VP_LV(QQ, SS, 14) VP_LV(QQ, SS, 15)
        VP_LVROW(q0, s0)
        if (p - 1 > 16) { VP_LVROW(q1, s1) }
        if (p - 1 > 32) { VP_LVROW(q2, s2) }
#undef VP_LVROW
#undef VP_LV
        const double k = (rp - rho_a) / (r0 - r_a);
        const double pa0 = (c == 0) ? P0 : (c == 1) ? P1 : P2;                // register c - 0
        const double pa1 = (c == 1) ? P0 : P1;                                // register c - 1 (c is 1 or 2 wherever in1 holds)
        double n0 = A0, n1 = A1, n2 = A2;
        if (in0) n0 = A0 - k * pa0;
        if (in1) n1 = A1 - k * pa1;
        if (in2) n2 = A2 - k * P0;                                           // (c is 2 wherever in2 holds)
        if (i0 == p) n0 = k;
        if (i1 == p) n1 = k;
        if (i2 == p) n2 = k;
        A0 = n0; A1 = n1; A2 = n2;
    }
    if (lane == 0) a[0] = 1.0;
    if (i0 <= order) a[i0] = A0 * -1.;                                        // :145-146 (the four rows store the same values)
    if (i1 <= order) a[i1] = A1 * -1.;
    if (i2 <= order) a[i2] = A2 * -1.;
    return false;
}

// VP_IIR_FAST (where the autocorrelation is tolerance-mode arithmetic already: autocorr_rows_fast), orders 16..63: the recursion
// with ONE slot per lane (lane l holds a[l + 1]) and everything an order step needs moved by DPP instead of fetched:
//  * the two sums are lane-parallel products and a reduction tree (four row rotations, two row broadcasts, one readlane) instead
//    of chains of up to 48 dependent additions -- not the reference's summation order;
//  * Q[i] = r[p - i] and B[i] = a[p - i] (the partner of a[i] in the update) ride along in the same lanes and move ONE LANE per
//    step: a'[p + 1 - i] = B[i - 1] - k A[i - 1] is the very operation the update performs for that entry, so the next step's B
//    is (B - k A) shifted up by one lane with B'[1] = k, and Q shifts up with Q'[1] = r[p] (wave_shr:1; no shuffles, no LDS).
// A single wavefront is bound by instruction ISSUE here (every VALU instruction of a wave64 takes four cycles whatever it does):
// the three-register row form (levinson_row48) issues ~200 instructions per order step, this one ~70 -- 20 -> 6 us at order 48.
template <class RP, class AP>
__device__ __forceinline__ bool levinson_fast64(RP r, AP a, int order_, int aLen, double eps)
{
    const int lane = vp_tid() & 63;
    const int order = __builtin_amdgcn_readfirstlane(order_);
    if (fabs(r[0]) < eps) {                        // :110-114
        for (int i = lane; i < aLen; i += WAVE) a[i] = (i == 0) ? 1.0 : 0.0;
        return true;
    }
    const double r0 = r[0];
    const int i = lane + 1;
    double A = 0.0;                                                           // a[i]
    if (lane == 0) A = r[1] / r0;
    const double R = (i <= order) ? r[i] : 0.0;
    double Q = (lane == 0) ? r[1] : 0.0, B = A;                               // p = 2: Q[1] = r[1], B[1] = a[1]
    auto dpp = [](double v, auto ctrl, auto rowMask) -> double {
        return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), decltype(ctrl)::value, decltype(rowMask)::value, 0xf, false),
                                __builtin_amdgcn_update_dpp(0, __double2loint(v), decltype(ctrl)::value, decltype(rowMask)::value, 0xf, false));
    };
#define VP_DPP(V, CTRL, MASK) dpp(V, std::integral_constant<int, CTRL>{}, std::integral_constant<int, MASK>{})
    for (int p = 2; p <= order; p++) {
        double rho = Q * A, ra = R * A;                                       // (a beyond p - 1 is +0.0, Q and R are finite)
        const double rp = bcast_f64(R, p - 1);                                // r[p] sits in lane p - 1
        rho += VP_DPP(rho, 0x128, 0xf); ra += VP_DPP(ra, 0x128, 0xf);         // row_ror:8
        rho += VP_DPP(rho, 0x124, 0xf); ra += VP_DPP(ra, 0x124, 0xf);         // row_ror:4
        rho += VP_DPP(rho, 0x122, 0xf); ra += VP_DPP(ra, 0x122, 0xf);         // row_ror:2
        rho += VP_DPP(rho, 0x121, 0xf); ra += VP_DPP(ra, 0x121, 0xf);         // row_ror:1: every lane holds its row's totals
        rho += VP_DPP(rho, 0x142, 0xa); ra += VP_DPP(ra, 0x142, 0xa);         // row_bcast:15 -> rows 1 and 3
        rho += VP_DPP(rho, 0x143, 0xc); ra += VP_DPP(ra, 0x143, 0xc);         // row_bcast:31 -> rows 2 and 3: lane 63 holds the wave's totals
        const double k = (rp - bcast_f64(rho, 63)) / (r0 - bcast_f64(ra, 63));
        double n = A - k * B;
        const double t = B - k * A;
        if (i == p) n = k;
        if (i > p) n = 0.0;
        A = n;
        B = VP_DPP(t, 0x138, 0xf);                                            // wave_shr:1
        Q = VP_DPP(Q, 0x138, 0xf);
        if (lane == 0) { B = k; Q = rp; }
        if (i > p) B = 0.0;
    }
#undef VP_DPP
    if (lane == 0) a[0] = 1.0;
    if (i <= order) a[i] = A * -1.;                                           // :145-146
    return false;
}

// Levinson-Durbin for orders 16..P by ONE wavefront with every lane running the whole recursion (LPC.cpp:107-148 as it
// stands), the autocorrelation and coefficient vectors in REGISTERS (fully unrolled, static names).  Sixty-four lanes doing
// the same thing is as wasteful as it sounds, but the wave-distributed form above pays two LDS round trips per order step
// for its ordered sums (26 us at order 40, 42 us at order 48); this one has none and takes a quarter of that.
// r, a: LDS vectors.  Returns true when the whole vector was rewritten (the |r0| < eps branch).
// (not inlined: the body is ~8000 instructions and the kernels call it from several places)
template <int P>
__device__ __noinline__ bool levinson_scalar(const lds_f64 *r, lds_f64 *a, int order_, int aLen, double eps)
{
    const int lane = vp_tid() & 63;
    const int order = __builtin_amdgcn_readfirstlane(order_);
    if (fabs(r[0]) < eps) {                        // :110-114
        for (int i = lane; i < aLen; i += WAVE) a[i] = (i == 0) ? 1.0 : 0.0;
        return true;
    }
    double rr[P + 1], aa[P + 1];
#pragma unroll
    for (int k = 0; k <= P; k++) { rr[k] = (k <= order) ? r[k] : 0.0; aa[k] = 0.0; }
    const double r0 = rr[0];
    aa[0] = 1.0;
    aa[1] = rr[1] / r0;
#pragma unroll
    for (int p = 2; p <= P; p++) {
        if (p <= order) {                          // wave-uniform
            double rho_a = 0.0, r_a = 0.0;
#pragma unroll
            for (int i = 1; i < p; i++) {          // :120-128
                rho_a += rr[p - i] * aa[i];
                r_a += rr[i] * aa[i];
            }
            const double k = (rr[p] - rho_a) / (r0 - r_a);
#pragma unroll
            for (int i = 1; 2 * i <= p; i++) {     // a[i] = aPrev[i] - k aPrev[p-i], both ends of the pair
                const double ai = aa[i], aj = aa[p - i];
                aa[i] = ai - k * aj;
                if (2 * i != p) aa[p - i] = aj - k * ai;
            }
            aa[p] = k;
        }
    }
    if (lane == 0) a[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= P; k++)
        if (k <= order && lane == (k & 63)) a[k] = aa[k] * -1.;             // :145-146
    return false;
}

// The same register-resident recursion with one WINDOW per lane (r, a: the lane's own vectors; the order is wave-uniform):
// the workgroup vocoder's round of up to eight windows on ONE wavefront instead of eight wavefronts that each run it 64 times
// over (they share four SIMDs and an LDS pipe: 27 us per round at order 40 for the wave-distributed form).  A lane whose
// r[0] is below eps writes the unit vector (LPC.cpp:110-114) and steps out.
// FS (VP_IIR_FAST): sums and updates as fused multiply-adds (half the instructions of a fetch-bound, fully unrolled recursion)
template <int P, bool FS = false>
__device__ __forceinline__ void levinson_lanes_inl(const lds_f64 *r, lds_f64 *a, int order_, int aLen, double eps)
{
    const int order = __builtin_amdgcn_readfirstlane(order_);
    double rr[P + 1], aa[P + 1];
#pragma unroll
    for (int k = 0; k <= P; k++) { rr[k] = (k <= order) ? r[k] : 0.0; aa[k] = 0.0; }
    const double r0 = rr[0];
    if (fabs(r0) < eps) {
        for (int i = 0; i < aLen; i++) a[i] = (i == 0) ? 1.0 : 0.0;
        return;
    }
    aa[0] = 1.0;
    aa[1] = rr[1] / r0;
#pragma unroll
    for (int p = 2; p <= P; p++) {
        if (p <= order) {                          // wave-uniform
            double rho_a = 0.0, r_a = 0.0;
#pragma unroll
            for (int i = 1; i < p; i++) {          // :120-128
                if (FS) { rho_a = __builtin_fma(rr[p - i], aa[i], rho_a); r_a = __builtin_fma(rr[i], aa[i], r_a); }
                else {
                rho_a += rr[p - i] * aa[i];
                r_a += rr[i] * aa[i];
                }
            }
            const double k = (rr[p] - rho_a) / (r0 - r_a);
#pragma unroll
            for (int i = 1; 2 * i <= p; i++) {     // a[i] = aPrev[i] - k aPrev[p-i], both ends of the pair
                const double ai = aa[i], aj = aa[p - i];
                if (FS) { aa[i] = __builtin_fma(-k, aj, ai); if (2 * i != p) aa[p - i] = __builtin_fma(-k, ai, aj); }
                else {
                aa[i] = ai - k * aj;
                if (2 * i != p) aa[p - i] = aj - k * ai;
                }
            }
            aa[p] = k;
        }
    }
    a[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= P; k++)
        if (k <= order) a[k] = aa[k] * -1.;                                  // :145-146
}
// (as a real call: the P = 48 body is ~8000 instructions and 200 VGPRs; smaller ones are inlined by their callers)
template <int P, bool FS = false>
__device__ __noinline__ void levinson_lanes(const lds_f64 *r, lds_f64 *a, int order_, int aLen, double eps)
{
    levinson_lanes_inl<P, FS>(r, a, order_, aLen, eps);
}

// Left-to-right sums of e[i]^2 for two arrays at once (VocoderProcess.cpp:250), every lane of the
// calling wavefront redundantly: eight entries are read ahead per trip so that only the two
// (interleaved) chains of dependent adds remain.
template <class EP>
__device__ __forceinline__ void energy_pair_wave(EP e0, EP e1, int n, double &E0, double &E1)
{
    double r0 = 0.0, r1 = 0.0;
    if ((n & 15) == 0) {
        // sixteen entries per trip: ONE read per array (lane l holds entry i + (l & 15), every 16-lane
        // row the same), the squares computed once, lane-parallel, and the two ordered sums taken as
        // chains of v_fmac_f64 with a DPP row-broadcast operand (x * 1.0 + run rounds like run + x).
        // Per element this is two VALU ops and an eighth of an LDS read instead of two loads, two
        // multiplies and two adds done redundantly by every lane.
        const int l16 = vp_tid() & 15;
        const double one = vp_one();
        double v0 = e0[l16], v1 = e1[l16];
        for (int i = 0; i < n; i += 16) {
            double s0 = v0 * v0, s1 = v1 * v1;
            if (i + 16 < n) { v0 = e0[i + 16 + l16]; v1 = e1[i + 16 + l16]; }
            asm volatile("s_nop 1" : "+v"(s0), "+v"(s1));                      // VALU write -> DPP read
#define VP_EN(U) VP_FMAC_BCAST(r0, s0, one, U); VP_FMAC_BCAST(r1, s1, one, U);
            VP_EN(0) VP_EN(1) VP_EN(2) VP_EN(3) VP_EN(4) VP_EN(5) VP_EN(6) VP_EN(7)
            VP_EN(8) VP_EN(9) VP_EN(10) VP_EN(11) VP_EN(12) VP_EN(13) VP_EN(14) VP_EN(15)
#undef VP_EN
        }
        E0 = r0; E1 = r1;
        return;
    }
    const int n8 = n & ~7;
    for (int i = 0; i < n8; i += 8) {
        double a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { a[u] = e0[i + u]; b[u] = e1[i + u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) { a[u] = a[u] * a[u]; b[u] = b[u] * b[u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) { r0 += a[u]; r1 += b[u]; }
    }
    for (int i = n8; i < n; i++) { double a = e0[i], b = e1[i]; r0 += a * a; r1 += b * b; }
    E0 = r0; E1 = r1;
}

// One array's left-to-right sum of e[i]^2, same arithmetic as a half of energy_pair_wave (for callers that give the two
// sums to two wavefronts).
template <class EP>
__device__ __forceinline__ double energy_wave(EP e0, int n)
{
    double r0 = 0.0;
    if ((n & 15) == 0) {
        const int l16 = vp_tid() & 15;
        const double one = vp_one();
        double v0 = e0[l16];
        for (int i = 0; i < n; i += 16) {
            double s0 = v0 * v0;
            if (i + 16 < n) v0 = e0[i + 16 + l16];
            asm volatile("s_nop 1" : "+v"(s0));                                // VALU write -> DPP read
#define VP_EN(U) VP_FMAC_BCAST(r0, s0, one, U);
            VP_EN(0) VP_EN(1) VP_EN(2) VP_EN(3) VP_EN(4) VP_EN(5) VP_EN(6) VP_EN(7)
            VP_EN(8) VP_EN(9) VP_EN(10) VP_EN(11) VP_EN(12) VP_EN(13) VP_EN(14) VP_EN(15)
#undef VP_EN
        }
        return r0;
    }
    const int n8 = n & ~7;
    for (int i = 0; i < n8; i += 8) {
        double a[8];
#pragma unroll
        for (int u = 0; u < 8; u++) a[u] = e0[i + u];
#pragma unroll
        for (int u = 0; u < 8; u++) a[u] = a[u] * a[u];
#pragma unroll
        for (int u = 0; u < 8; u++) r0 += a[u];
    }
    for (int i = n8; i < n; i++) { double a = e0[i]; r0 += a * a; }
    return r0;
}

// VocoderProcess::filterFIR (VocoderProcess.cpp:235-251) for one window by one wavefront:
// e[i] = a[0]*xw[i] + sum_{k=1..min(order,i)} xw[i-k]*a[k].
// FS (VP_IIR_FAST): a tap is one fused multiply-add
template <bool FS = false, class XP, class AP, class EP>
__device__ __forceinline__ void fir_window8(XP xw, AP a, int order, int W, EP e, int lane, int unit0 = 0, int unitStep = 1)
{
    // units of 8 x 64 outputs; a caller that shares the window with other wavefronts takes units unit0, unit0 + unitStep, ...
    for (int i0 = unit0 * 8 * WAVE; i0 < W; i0 += unitStep * 8 * WAVE) {
        double acc[8];
        int idx[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            idx[u] = i0 + lane + u * WAVE;
            acc[u] = (idx[u] < W) ? a[0] * xw[idx[u]] : 0.0;             // a[0]*x*w with a[0] == 1
        }
        for (int k = 1; k <= order; k++) {
            const double ak = a[k];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int j = idx[u] - k;
                const double xv_ = (j >= 0 && idx[u] < W) ? xw[j] : 0.0;
                if (FS) acc[u] = __builtin_fma(xv_, ak, acc[u]); else acc[u] += xv_ * ak;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) if (idx[u] < W) e[idx[u]] = acc[u];
    }
}

// PitchProcess::filterFIR (PitchProcess.cpp:280-302) for FOUR consecutive outputs e[j0 .. j0+3] by one thread:
// e[j] = a[0] x[j] + sum_{k=1..min(order, j)} x[j-k] a[k], every output summed in the reference's order k = 1, 2, ...
// The four outputs share the sliding window of inputs (one new x and one coefficient per tap for eight operations,
// four independent chains) instead of two LDS reads per multiply-add.  x points at the sample of output 0 of the
// whole filter call (so that j - k >= 0 is the history test), eo at its output.
// SEL: the caller may hand over outputs whose history is shorter than the order (see below; compiled in for that one call site)
template <bool SEL = false>
__device__ __forceinline__ void fir4(const lds_f64 *x, const lds_f64 *a, int order, int j0, int jEnd, lds_f64 *eo)
{
    if (j0 >= jEnd) return;
    if (j0 >= order && j0 + 4 <= jEnd) {
        double w0 = x[j0], w1 = x[j0 + 1], w2 = x[j0 + 2], w3 = x[j0 + 3];
        const double a0 = a[0];
        double e0 = a0 * w0, e1 = a0 * w1, e2 = a0 * w2, e3 = a0 * w3;
        int k = 1;
        for (; k + 3 <= order; k += 4) {                                     // four taps per trip, window registers rotate by name
            const double ak0 = a[k], ak1 = a[k + 1], ak2 = a[k + 2], ak3 = a[k + 3];
            const double n0 = x[j0 - k], n1 = x[j0 - k - 1], n2 = x[j0 - k - 2], n3 = x[j0 - k - 3];
            e0 += n0 * ak0; e1 += w0 * ak0; e2 += w1 * ak0; e3 += w2 * ak0;   // tap k:   x[j-k] for j = j0..j0+3
            e0 += n1 * ak1; e1 += n0 * ak1; e2 += w0 * ak1; e3 += w1 * ak1;   // tap k+1
            e0 += n2 * ak2; e1 += n1 * ak2; e2 += n0 * ak2; e3 += w0 * ak2;   // tap k+2
            e0 += n3 * ak3; e1 += n2 * ak3; e2 += n1 * ak3; e3 += n0 * ak3;   // tap k+3
            w3 = n0; w2 = n1; w1 = n2; w0 = n3;                               // the window is now x[j0-k-3 .. j0-k]
        }
        for (; k <= order; k++) {
            const double ak = a[k], n0 = x[j0 - k];
            e0 += n0 * ak; e1 += w0 * ak; e2 += w1 * ak; e3 += w2 * ak;
            w3 = w2; w2 = w1; w1 = w0; w0 = n0;
        }
        eo[j0] = e0; eo[j0 + 1] = e1; eo[j0 + 2] = e2; eo[j0 + 3] = e3;
        return;
    }
    if (SEL && VP_FIR4_SELECT != 0 && j0 + 4 <= jEnd) {
        // the filter's first outputs (history shorter than the order): the same four chains and sliding window, a tap joining output
        // j's sum only while k <= j -- a select, not an addition of zero: the reference performs no operation there.  (The scalar
        // loop below paid two dependent LDS round trips per tap and output: 26 us for the first 48 outputs of an order-48 frame,
        // on a wavefront the whole workgroup then waited for.)
        double w0 = x[j0], w1 = x[j0 + 1], w2 = x[j0 + 2], w3 = x[j0 + 3];
        const double a0 = a[0];
        double e0 = a0 * w0, e1 = a0 * w1, e2 = a0 * w2, e3 = a0 * w3;
        const int kEnd = min(order, j0 + 3);
        for (int k = 1; k <= kEnd; k += 4) {
            double ak[4], n[4];
#pragma unroll
            for (int t = 0; t < 4; t++) { ak[t] = a[min(k + t, order)]; n[t] = x[max(j0 - k - t, 0)]; }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int kk = k + t;
                const double t0 = e0 + n[t] * ak[t], t1 = e1 + w0 * ak[t], t2 = e2 + w1 * ak[t], t3 = e3 + w2 * ak[t];
                const bool in = kk <= order;
                e0 = (in && kk <= j0) ? t0 : e0; e1 = (in && kk <= j0 + 1) ? t1 : e1;
                e2 = (in && kk <= j0 + 2) ? t2 : e2; e3 = (in && kk <= j0 + 3) ? t3 : e3;
                w3 = w2; w2 = w1; w1 = w0; w0 = n[t];
            }
        }
        eo[j0] = e0; eo[j0 + 1] = e1; eo[j0 + 2] = e2; eo[j0 + 3] = e3;
        return;
    }
    for (int j = j0; j < min(j0 + 4, jEnd); j++) {                           // ragged end
        double e = a[0] * x[j];
        const int kmax = min(order, j);
        for (int k = 1; k <= kmax; k++) e += x[j - k] * a[k];
        eo[j] = e;
    }
}

// v_mul_f64 / v_add_f64 with a pinned program order (asm volatile statements keep their relative
// order).  Measured on gfx950 (tools/ubench_chain2.hip): a dependent fp64 op completes in ~8 cycles,
// a wave can issue one every ~4, so a chain step costs 8 cycles provided the NEXT products are
// already in flight; hipcc's own schedule put each product right in front of its subtract
// (16 cycles per tap).  Plain VALU ops on VGPR operands: hardware interlocks cover the dependencies.
#define VP_MUL64(D, A, B) asm volatile("v_mul_f64 %0, %1, %2" : "=v"(D) : "v"(A), "v"(B))
#define VP_SUB64(ACC, T) asm volatile("v_add_f64 %0, %0, -%1" : "+v"(ACC) : "v"(T))
#define VP_COPY64(D, S) asm("v_mul_f64 %0, %1, 1.0" : "=v"(D) : "v"(S))

template <int P, class XP, class YP, class AP, class HP>
__device__ __forceinline__ void iir_exact_lane(XP x, YP y, int n, AP aL, int order, HP hist, double gmul)
{
    static_assert(P % 4 == 0 && P >= 4, "P multiple of 4");
    double a[P + 1], h[P + 4];
#pragma unroll
    for (int k = 1; k <= P; k++) a[k] = (k <= order) ? aL[k] : 0.0;
#pragma unroll
    for (int j = 0; j < P; j++) h[j] = (hist && j < order) ? hist[j] : 0.0;
    for (int i = 0; i < n; i += 4) {
        double yn[4];
        const double xin[4] = {x[i], x[i + 1], x[i + 2], x[i + 3]};
#pragma unroll
        for (int s2 = 0; s2 < 4; s2++) {
            // tap k multiplies y[i+s2-k]: one of this trip's fresh outputs (k <= s2) or history
#define VP_HV(K) (((K) <= s2) ? yn[s2 - (K) < 0 ? 0 : s2 - (K)] : h[(K) - 1 - s2])
            double acc = gmul * xin[s2];
            double t[3];
            VP_MUL64(t[2 % 3], VP_HV(2), a[2]);           // independent of the sample just finished
            VP_MUL64(t[3 % 3], VP_HV(3), a[3]);
            VP_MUL64(t[1 % 3], VP_HV(1), a[1]);           // needs y[i+s2-1]: the one unavoidable wait
#pragma unroll
            for (int k = 1; k <= P; k++) {
                VP_SUB64(acc, t[k % 3]);
                if (k + 3 <= P) VP_MUL64(t[k % 3], VP_HV(k + 3), a[k + 3]);   // refill the slot just consumed
            }
            yn[s2] = acc;
#undef VP_HV
        }
        // history shift.  A plain double copy compiles to v_mov_b64, measured at ~12 ns per wave
        // instruction on gfx950 (tools/ubench_chain.hip) against 1.9 ns for an fp64 multiply, so
        // the copies are written as exact multiplications by 1.0.
#pragma unroll
        for (int j = P - 1; j >= 4; j--) VP_COPY64(h[j], h[j - 4]);
        VP_COPY64(h[3], yn[0]); VP_COPY64(h[2], yn[1]); VP_COPY64(h[1], yn[2]); VP_COPY64(h[0], yn[3]);
        y[i] = yn[0]; y[i + 1] = yn[1]; y[i + 2] = yn[2]; y[i + 3] = yn[3];
    }
}

// Generic (any order, any n) form of the same recursion with the history read back from y[]:
// y must be preceded by its own past (y[-k] valid for k <= min(order, i0 + i)).
template <class XP, class YP, class AP>
__device__ __forceinline__ void iir_exact_generic(XP x, YP y, int n, AP aL, int order, int i0, double gmul)
{
    for (int i = 0; i < n; i++) {
        double acc = gmul * x[i];
        const int kmax = min(order, i0 + i);
        for (int k = 1; k <= kmax; k++) acc -= y[i - k] * aL[k];
        y[i] = acc;
    }
}

// Dispatch on the (wave-uniform) order.  hist as in iir_exact_lane; i0 = number of valid past
// outputs before y[0] (only used by the generic path).
// LITE = the register-light kernel variant (two workgroups per CU): only the small register-resident
// instantiations, larger orders take the generic LDS form.
// PMAX: largest register-resident instantiation this caller carries (a build that is only launched for smaller orders leaves
// the big ones -- 200 VGPRs at 48 -- out of its register allocation)
template <bool LITE = false, int PMAX = 48, class XP, class YP, class AP, class HP>
__device__ __forceinline__ void iir_exact(XP x, YP y, int n, AP aL, int order_, HP hist, int i0, double gmul)
{
    const int order = __builtin_amdgcn_readfirstlane(order_);
    const bool q = (__builtin_amdgcn_readfirstlane(n) & 3) == 0;
    if (q && order <= 8) iir_exact_lane<8>(x, y, n, aL, order, hist, gmul);
    else if (q && order <= 16) iir_exact_lane<16>(x, y, n, aL, order, hist, gmul);
    else if (LITE) iir_exact_generic(x, y, n, aL, order, i0, gmul);
    else if (q && order <= 24) iir_exact_lane<24>(x, y, n, aL, order, hist, gmul);
    else if (q && order <= 32) iir_exact_lane<32>(x, y, n, aL, order, hist, gmul);
    else if (PMAX >= 40 && q && order <= 40) iir_exact_lane<(PMAX >= 40 ? 40 : 8)>(x, y, n, aL, order, hist, gmul);
    else if (PMAX >= 48 && q && order <= 48) iir_exact_lane<(PMAX >= 48 ? 48 : 8)>(x, y, n, aL, order, hist, gmul);
    else iir_exact_generic(x, y, n, aL, order, i0, gmul);
}

// lane i <- lane i+1 of the whole wavefront (DPP wave_shl:1, a plain VALU move: no LDS round trip
// like ds_bpermute); lane 63 receives 0.
__device__ __forceinline__ double wave_shl1_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);       // (bound_ctrl: the lane without a source reads 0 -- no pre-zeroed
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);       // destination, two moves fewer per call)
    return __hiloint2double(hi, lo);
}

// FAST (not bit-exact) form of the same all-pole recursion, selected with vp_set_iir_mode(h, 1):
// transposed direct form II with the state vector spread over the lanes (lane j holds s_{j+1},
// and s_{j+65} for orders above 64):   y = g*x + s_1 ;  s_k = s_{k+1} - a_k*y  (one fma per lane).
// The critical path per sample is readlane -> add -> fma whatever the order, against (order+1)
// dependent operations for the exact chain.  The taps are summed oldest-first instead of
// newest-first, so the result differs from the reference's by rounding only (~1e-16 relative per
// operation); no decision of the algorithm depends on an IIR output.  hist[j] = y[-1-j] or nullptr.
template <bool TWO, class XP, class YP, class AP, class HP>
__device__ __forceinline__ void iir_fast_wave_impl(XP x, YP y, int n, AP aL, int order, HP hist, double gmul)
{
    const int lane = vp_tid() & 63;
    const int k0 = lane + 1, k1 = lane + 65;
    const double a0 = (k0 <= order) ? aL[k0] : 0.0;
    const double a1 = (TWO && k1 <= order) ? aL[k1] : 0.0;
    double s0 = 0.0, s1 = 0.0;
    if (hist) {                                   // state equivalent to the given output history
        for (int m = 0; m < order; m++) {
            const double hm = hist[m];
            if (k0 + m <= order) s0 = __builtin_fma(-aL[k0 + m], hm, s0);
            if (TWO && k1 + m <= order) s1 = __builtin_fma(-aL[k1 + m], hm, s1);
        }
    }
    auto step = [&](double xi) -> double {
        const double yy = __builtin_fma(gmul, xi, bcast_f64(s0, 0));
        double n0 = wave_shl1_f64(s0), n1 = 0.0;
        if (TWO) {
            const double c = bcast_f64(s1, 0);
            n1 = wave_shl1_f64(s1);
            if (lane == 63) n0 = c;
        }
        s0 = __builtin_fma(-a0, yy, n0);
        if (TWO) s1 = __builtin_fma(-a1, yy, n1);
        return yy;
    };
    const int n8 = n & ~7;
    for (int i = 0; i < n8; i += 8) {
        double xv[8], yv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) xv[u] = x[i + u];
#pragma unroll
        for (int u = 0; u < 8; u++) yv[u] = step(xv[u]);
#pragma unroll
        for (int u = 0; u < 8; u++) y[i + u] = yv[u];           // every lane stores the same value
    }
    for (int i = n8; i < n; i++) y[i] = step(x[i]);
}
template <class XP, class YP, class AP, class HP>
__device__ __forceinline__ void iir_fast_wave(XP x, YP y, int n, AP aL, int order_, HP hist, double gmul)
{
    const int order = __builtin_amdgcn_readfirstlane(order_);
    if (order > 64) iir_fast_wave_impl<true>(x, y, n, aL, order, hist, gmul);
    else iir_fast_wave_impl<false>(x, y, n, aL, order, hist, gmul);
}

// FAST mode, BLOCK form of the all-pole recursion (used when n is a multiple of 64): with h the
// impulse response of 1/A(z) (64 samples, computed once per coefficient set with the wave recursion
// above), a block of 64 outputs is   y = T(h) (g x + u),   u_i = -sum_{m>i} a_m y[i-m]  (i < order)
// carrying the previous outputs in, T(h) lower-triangular Toeplitz.  One lane per output sample:
// no dependence between the samples of a block, ~0.4 us per block instead of 64 x 33 ns.
// hpad: 128 doubles (64 zeros, then h), xp: 64 doubles of scratch.  nh0 = valid outputs before y[0].
template <class XP, class YP, class AP>
__device__ __forceinline__ void iir_block_wave(XP x, YP y, int n, AP aL, int order_, int nh0, const lds_f64 *hpad, lds_f64 *xp,
                                               double gmul)
{
    const int lane = vp_tid() & 63;
    const int order = __builtin_amdgcn_readfirstlane(order_);
    for (int b = 0; b < n; b += WAVE) {
        STAMPG_BEGIN();
        // u_lane = -sum_{k=1..order} a[lane+k] * y[b-k]   (a beyond the order = 0; y before the start = 0):
        // the history values are wave-uniform reads, the trip count is uniform, two accumulators
        const int kmax = (b == 0) ? min(order, nh0) : order;
        double u0 = 0.0, u1 = 0.0;
        int k = 1;
        // eight taps per trip, their sixteen LDS reads issued together (the two-tap loop this replaces waited out an LDS
        // round trip per pair: 1.8 us per 64-sample block at order 48, 79 of the IIR's 92 us per block at the configs[4] geometry)
        for (; k + 7 <= kmax; k += 8) {
            double yv[8], av[8];
#pragma unroll
            for (int t = 0; t < 8; t++) { yv[t] = y[b - k - t]; av[t] = (lane + k + t <= order) ? aL[lane + k + t] : 0.0; }
#pragma unroll
            for (int t = 0; t < 8; t += 2) { u0 = __builtin_fma(-av[t], yv[t], u0); u1 = __builtin_fma(-av[t + 1], yv[t + 1], u1); }
        }
        for (; k + 1 <= kmax; k += 2) {
            const double y1 = y[b - k], y2 = y[b - k - 1];
            const double a1 = (lane + k <= order) ? aL[lane + k] : 0.0;
            const double a2 = (lane + k + 1 <= order) ? aL[lane + k + 1] : 0.0;
            u0 = __builtin_fma(-a1, y1, u0);
            u1 = __builtin_fma(-a2, y2, u1);
        }
        if (k <= kmax) { const double a1 = (lane + k <= order) ? aL[lane + k] : 0.0; u0 = __builtin_fma(-a1, y[b - k], u0); }
        const double u = u0 + u1;
        xp[lane] = __builtin_fma(gmul, x[b + lane], u);
        STAMPG(24);
        // 64-term dot product with four independent accumulators, eight terms read ahead per trip
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        const lds_f64 *hh = hpad + WAVE + lane;                             // hh[-j] = h[lane - j] (0 for j > lane)
        double hv[8], xv[8], hn[8], xn[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { hv[q] = hh[-q]; xv[q] = xp[q]; }
#pragma unroll
        for (int j = 0; j < WAVE; j += 8) {
            if (j + 8 < WAVE) {
#pragma unroll
                for (int q = 0; q < 8; q++) { hn[q] = hh[-(j + 8 + q)]; xn[q] = xp[j + 8 + q]; }
            }
            acc0 = __builtin_fma(hv[0], xv[0], acc0); acc1 = __builtin_fma(hv[1], xv[1], acc1);
            acc2 = __builtin_fma(hv[2], xv[2], acc2); acc3 = __builtin_fma(hv[3], xv[3], acc3);
            acc0 = __builtin_fma(hv[4], xv[4], acc0); acc1 = __builtin_fma(hv[5], xv[5], acc1);
            acc2 = __builtin_fma(hv[6], xv[6], acc2); acc3 = __builtin_fma(hv[7], xv[7], acc3);
#pragma unroll
            for (int q = 0; q < 8; q++) { hv[q] = hn[q]; xv[q] = xn[q]; }
        }
        const double acc = (acc0 + acc1) + (acc2 + acc3);
        y[b + lane] = acc;
        STAMPG(25);
    }
}

// The same block form with the dot product kept off the LDS (orders <= 16, whole 64-sample blocks,
// called by ONE full wavefront).  A DS instruction costs its wave 4-8 ns of issue even when nothing
// waits for it (tools/ubench_lds.hip), and the LDS form above spends two of them per term.  Here
//   * the lane's 64 taps H[j] = h[lane - j] stay in registers for the whole chunk (128 VGPRs),
//   * the block's input is held as four registers X_q[lane] = x[b + 16 q + (lane & 15)] (every
//     16-lane row holds the same 16 samples), so that term i = 16 q + m is ONE instruction,
//     v_fmac_f64_dpp acc, X_q row_newbcast:m, H[i], with no broadcast traffic at all,
//   * the carry-in of the previous block only reaches samples 0..order-1 <= 15, i.e. X_0: each row
//     computes it for its own copy, and the 48 terms of X_1..X_3 are issued while the history
//     values (the previous block's last outputs, written a moment ago) come back from the LDS.
// Rounding differs from the LDS form only in the order of the partial sums (both are FAST mode).
#define VP_BI_T(ACC, XQ, HI, M) \
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #M " row_mask:0xf bank_mask:0xf" : "+v"(ACC) : "v"(XQ), "v"(HI))
#define VP_BI_ROW(XQ, Q) \
    VP_BI_T(acc0, XQ, H[16 * Q + 0], 0);   VP_BI_T(acc1, XQ, H[16 * Q + 1], 1);   VP_BI_T(acc2, XQ, H[16 * Q + 2], 2);   \
    VP_BI_T(acc3, XQ, H[16 * Q + 3], 3);   VP_BI_T(acc0, XQ, H[16 * Q + 4], 4);   VP_BI_T(acc1, XQ, H[16 * Q + 5], 5);   \
    VP_BI_T(acc2, XQ, H[16 * Q + 6], 6);   VP_BI_T(acc3, XQ, H[16 * Q + 7], 7);   VP_BI_T(acc0, XQ, H[16 * Q + 8], 8);   \
    VP_BI_T(acc1, XQ, H[16 * Q + 9], 9);   VP_BI_T(acc2, XQ, H[16 * Q + 10], 10); VP_BI_T(acc3, XQ, H[16 * Q + 11], 11); \
    VP_BI_T(acc0, XQ, H[16 * Q + 12], 12); VP_BI_T(acc1, XQ, H[16 * Q + 13], 13); VP_BI_T(acc2, XQ, H[16 * Q + 14], 14); \
    VP_BI_T(acc3, XQ, H[16 * Q + 15], 15);
// RAGGED (round 6): n need not be a multiple of 64 -- the plugin's own geometry at 48 kHz has chunks of 278 samples
// (PluginProcessor.cpp:159-173), which until then took the sample-by-sample transposed form: 34 of that block's 99 us.  The last
// block's lanes beyond n read zeros and store nothing (what lies behind the chunk in x and y is the next chunk's, or the end of the
// frame's buffers); a lane's output depends on the block's earlier samples only, so the valid lanes compute what they always do.
template <bool RAGGED = false>
__device__ __forceinline__ void iir_block_wave_regs(const lds_f64 *x, lds_f64 *y, int n, const lds_f64 *aL, int order_,
                                                    bool haveHist0, const lds_f64 *hpad)
{
    const int lane = vp_tid() & 63, m = lane & 15;
    const int order = __builtin_amdgcn_readfirstlane(order_);
    // Two passes (round 3).  With all 64 taps resident this routine was the register peak of the whole pitch kernel (128 VGPRs
    // of taps: 255 in use, and every later addition to the kernel spilled).  Pass 1 -- the 48 terms of samples 16..63 of every
    // block, which depend on no earlier output -- runs over the whole chunk first with taps 16..63 resident and parks its sums
    // in y[] itself; pass 2 walks the blocks with taps 0..15 and the 16 history coefficients resident.  Same terms; the only
    // difference to the one-pass form is where the partial sums are joined (FAST-mode rounding).
    {
        double H[64];
#pragma unroll
        for (int j = 16; j < 64; j++) H[j] = hpad[WAVE + lane - j];           // h[lane - j], 0 for j > lane
        for (int b = 0; b < n; b += WAVE) {
            double X1 = x[RAGGED ? min(b + 16 + m, n - 1) : b + 16 + m], X2 = x[RAGGED ? min(b + 32 + m, n - 1) : b + 32 + m], X3 = x[RAGGED ? min(b + 48 + m, n - 1) : b + 48 + m];
            if (RAGGED) { X1 = (b + 16 + m < n) ? X1 : 0.0; X2 = (b + 32 + m < n) ? X2 : 0.0; X3 = (b + 48 + m < n) ? X3 : 0.0; asm volatile("s_nop 1" : "+v"(X1), "+v"(X2), "+v"(X3)); }
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
            VP_BI_ROW(X1, 1)
            VP_BI_ROW(X2, 2)
            VP_BI_ROW(X3, 3)
            if (!RAGGED || b + lane < n) y[b + lane] = (acc0 + acc1) + (acc2 + acc3);
        }
    }
    double H[16], A[16];
#pragma unroll
    for (int j = 0; j < 16; j++) H[j] = hpad[WAVE + lane - j];
#pragma unroll
    for (int k = 1; k <= 16; k++) A[k - 1] = (m + k <= order) ? -aL[m + k] : 0.0;  // -a[m + k]
    double X0 = (!RAGGED || m < n) ? x[RAGGED ? min(m, n - 1) : m] : 0.0;
    for (int b = 0; b < n; b += WAVE) {
        // history: Y3[lane] = y[b - 16 + (lane & 15)] (zero before the frame's first sample), so that
        // y[b - k] is lane 16 - k of the row
        const bool hist = (b > 0) || haveHist0;
        double Y3 = 0.0;
        // (only the last `order` outputs are history: older ones are not even restored when the frame continues in a
        // later launch, and a zero coefficient does not neutralise a NaN left in LDS by somebody else)
        if (hist && 16 - m <= order) Y3 = y[b - 16 + m];
        const double parked = (!RAGGED || b + lane < n) ? y[RAGGED ? min(b + lane, n - 1) : b + lane] : 0.0;
        double u0 = 0.0, u1 = 0.0;
        VP_BI_T(u0, Y3, A[0], 15);  VP_BI_T(u1, Y3, A[1], 14);  VP_BI_T(u0, Y3, A[2], 13);  VP_BI_T(u1, Y3, A[3], 12);
        VP_BI_T(u0, Y3, A[4], 11);  VP_BI_T(u1, Y3, A[5], 10);  VP_BI_T(u0, Y3, A[6], 9);   VP_BI_T(u1, Y3, A[7], 8);
        VP_BI_T(u0, Y3, A[8], 7);   VP_BI_T(u1, Y3, A[9], 6);   VP_BI_T(u0, Y3, A[10], 5);  VP_BI_T(u1, Y3, A[11], 4);
        VP_BI_T(u0, Y3, A[12], 3);  VP_BI_T(u1, Y3, A[13], 2);  VP_BI_T(u0, Y3, A[14], 1);  VP_BI_T(u1, Y3, A[15], 0);
        X0 = X0 + (u0 + u1);
        asm volatile("s_nop 1" : "+v"(X0));                                   // VALU write of X0 -> DPP read: 2 wait states
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        VP_BI_ROW(X0, 0)
        if (!RAGGED || b + lane < n) y[b + lane] = parked + ((acc0 + acc1) + (acc2 + acc3));
        const int bn = b + WAVE;
        if (bn < n) X0 = (!RAGGED || bn + m < n) ? x[RAGGED ? min(bn + m, n - 1) : bn + m] : 0.0;
    }
}

// The two passes of iir_block_wave_regs as routines of their own (whole 64-sample blocks), so that the wave-specialised kernel's
// producers can park pass 1 block by block behind their gather trips and the recursion wavefront is left with the walk: the same
// terms into the same accumulators, joined in the same places -- the output is iir_block_wave_regs' bit for bit (which stays the
// definition: the phase kernels call it).
// Pass 1 of ONE block: the 48 terms of samples b + 16 .. b + 63, parked in y[b + lane].  One full wavefront.
__device__ __forceinline__ void iir_block_park(const lds_f64 *x, lds_f64 *y, int b, const lds_f64 *hpad)
{
    const int lane = vp_tid() & 63, m = lane & 15;
    double H[64];
#pragma unroll
    for (int j = 16; j < 48; j++) H[j] = hpad[WAVE + lane - j];               // h[lane - j], 0 for j > lane
    const double X1 = x[b + 16 + m], X2 = x[b + 32 + m], X3 = x[b + 48 + m];
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    VP_BI_ROW(X1, 1)
    // (the caller runs this between two gather trips, with the trips' state in registers: the last sixteen taps are requested only now,
    // into the first row's registers -- 64 registers of taps at the peak instead of 96 -- and arrive while the second row is summed)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 48; j < 64; j++) H[j] = hpad[WAVE + lane - j];
    VP_BI_ROW(X2, 2)
    VP_BI_ROW(X3, 3)
    y[b + lane] = (acc0 + acc1) + (acc2 + acc3);
}
// Pass 2's registers: taps 0..15 and the 16 history coefficients.  They are the FRAME's, so the caller may request them ahead of
// the chunk (and keep them from chunk to chunk of one frame).
struct IirWalkRegs { double H[16], A[16]; };
__device__ __forceinline__ void iir_block_walk_load(IirWalkRegs &R, const lds_f64 *aL, int order_, const lds_f64 *hpad)
{
    const int lane = vp_tid() & 63, m = lane & 15;
    const int order = __builtin_amdgcn_readfirstlane(order_);
#pragma unroll
    for (int j = 0; j < 16; j++) R.H[j] = hpad[WAVE + lane - j];
#pragma unroll
    for (int k = 1; k <= 16; k++) R.A[k - 1] = (m + k <= order) ? -aL[m + k] : 0.0;  // -a[m + k]
}
// Pass 2 over a chunk whose blocks are all parked in y[] (iir_block_park).  One full wavefront.
__device__ __forceinline__ void iir_block_walk(const IirWalkRegs &R, const lds_f64 *x, lds_f64 *y, int n, int order_, bool haveHist0)
{
    const int lane = vp_tid() & 63, m = lane & 15;
    const int order = __builtin_amdgcn_readfirstlane(order_);
    double H[16], A[16];
#pragma unroll
    for (int j = 0; j < 16; j++) { H[j] = R.H[j]; A[j] = R.A[j]; }
    double X0 = x[m];
    for (int b = 0; b < n; b += WAVE) {
        const bool hist = (b > 0) || haveHist0;
        double Y3 = 0.0;
        if (hist && 16 - m <= order) Y3 = y[b - 16 + m];
        const double parked = y[b + lane];
        double u0 = 0.0, u1 = 0.0;
        VP_BI_T(u0, Y3, A[0], 15);  VP_BI_T(u1, Y3, A[1], 14);  VP_BI_T(u0, Y3, A[2], 13);  VP_BI_T(u1, Y3, A[3], 12);
        VP_BI_T(u0, Y3, A[4], 11);  VP_BI_T(u1, Y3, A[5], 10);  VP_BI_T(u0, Y3, A[6], 9);   VP_BI_T(u1, Y3, A[7], 8);
        VP_BI_T(u0, Y3, A[8], 7);   VP_BI_T(u1, Y3, A[9], 6);   VP_BI_T(u0, Y3, A[10], 5);  VP_BI_T(u1, Y3, A[11], 4);
        VP_BI_T(u0, Y3, A[12], 3);  VP_BI_T(u1, Y3, A[13], 2);  VP_BI_T(u0, Y3, A[14], 1);  VP_BI_T(u1, Y3, A[15], 0);
        X0 = X0 + (u0 + u1);
        asm volatile("s_nop 1" : "+v"(X0));                                   // VALU write of X0 -> DPP read: 2 wait states
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        VP_BI_ROW(X0, 0)
        y[b + lane] = parked + ((acc0 + acc1) + (acc2 + acc3));
        const int bn = b + WAVE;
        if (bn < n) X0 = x[bn + m];
    }
}

// The block form for orders 17..48 (whole 64-sample blocks, ONE full wavefront), with the recursion between the blocks
// reduced to what really is serial.  By linearity a block's outputs are
//     y[b + i] = z[b + i] + sum_{k=1..order} Hc[i][k] * y[b - k],        z = T(h) (g x)   (zero-state response),
// where column k of Hc is the block's response to a unit in history slot k.  Phase 1 computes z for ALL blocks of the chunk
// (no dependence between them: 64 DPP terms per block, taps in registers as above).  Phase 2 walks the blocks with the
// lane's row Hc[lane][1..48] in registers and the last 48 outputs in three row-broadcast registers: `order` DPP terms and
// one LDS round trip per 64 samples (the LDS form above: 112 terms with two LDS reads each, 2.3 us per block at order 48).
// Hc comes from the impulse response without any sum over taps:  Hc[i][1] = h[i+1],  Hc[i][k+1] = Hc[i+1][k] + a[k] h[i+1]
// (shift the carry-in sequence u_k[j] = -a[j+k] left by one), i.e. 47 steps of "lane i takes lane i+1's value" on h[0..111]:
// hpad holds 64 zeros, then h[0..127].  nh0 = valid outputs before y[0].  Rounding differs from the other FAST forms only
// in how the same sums are grouped.
// RN: history columns held in registers (a build that is only launched for orders up to 32 carries 32 of them)
// The two phases are separate functions so that two wavefronts can share a chunk: iir_hc_phase1 (the zero-state responses) on one,
// the history matrix and then -- once `flag` shows the generation number `gen`, raised by the other -- the walk on the calling one.
__device__ __forceinline__ void iir_hc_phase1(const lds_f64 *x, lds_f64 *y, int n, const lds_f64 *hpad, double gmul)
{
    const int lane = vp_tid() & 63, m = lane & 15;
    {
        double H[64];
#pragma unroll
        for (int j = 0; j < 64; j++) H[j] = hpad[WAVE + lane - j];            // h[lane - j], 0 for j > lane
        for (int b = 0; b < n; b += WAVE) {
            double X0 = gmul * x[b + m], X1 = gmul * x[b + 16 + m], X2 = gmul * x[b + 32 + m], X3 = gmul * x[b + 48 + m];
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
            asm volatile("s_nop 1" : "+v"(X0), "+v"(X1), "+v"(X2), "+v"(X3));     // VALU write -> DPP read
            VP_BI_ROW(X0, 0)
            VP_BI_ROW(X1, 1)
            VP_BI_ROW(X2, 2)
            VP_BI_ROW(X3, 3)
            y[b + lane] = (acc0 + acc1) + (acc2 + acc3);
        }
    }
}
template <int RN = 48>
__device__ __forceinline__ void iir_hc_phase2(lds_f64 *y, int n, const lds_f64 *aL, int order_, int nh0, const lds_f64 *hpad,
                                              int *flag = nullptr, int gen = 0, const VpTmo *timeouts = nullptr)
{
    static_assert(RN == 32 || RN == 48, "32 or 48 history columns");
    const int lane = vp_tid() & 63, m = lane & 15;
    const int order = __builtin_amdgcn_readfirstlane(order_);
    STAMPG_BEGIN();
    double R[RN];
    {
        const lds_f64 *h = hpad + WAVE;
        const double h0 = h[lane + 1], h1 = (lane + 65 < 128) ? h[lane + 65] : 0.0;   // h[i + 1] for i = lane, lane + 64
        double c0 = h0, c1 = h1;
        R[0] = c0;
        const double areg = (lane + 1 <= order) ? aL[lane + 1] : 0.0;         // a[k] in lane k - 1: ONE read, then readlanes (an LDS read
#pragma unroll                                                                // per step sat on the chain: 83 -> 47 ns per step)
        for (int k = 1; k < RN; k++) {
            const double ak = bcast_f64(areg, k - 1);
            const double up = bcast_f64(c1, 0);
            double n0 = wave_shl1_f64(c0);
            const double n1 = wave_shl1_f64(c1);
            if (lane == 63) n0 = up;
            c0 = __builtin_fma(ak, h0, n0);
            c1 = __builtin_fma(ak, h1, n1);
            R[k] = c0;
        }
    }
    STAMPG(24);
    if (flag) {                                       // the zero-state responses are another wavefront's work: wait for them
        int spin = 0;                                 // (bounded: a bug shows as a parity failure and a count, never as a hang)
        const int lim = timeouts ? timeouts->limit : (1 << 22);
        for (; spin < lim && __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != gen; spin++)
            __builtin_amdgcn_s_sleep(1);
        if (spin == lim && lane == 0 && timeouts) vp_timeout(*timeouts);
    }
    STAMPG(13);
    for (int b = 0; b < n; b += WAVE) {
        // Yq[lane] = y[b - 16 (4 - q) + (lane & 15)]: history slot k = 16 (4 - q) - m sits in lane 16 (4 - q) - k of the row.
        // Slots beyond the order, or before the frame's first sample, read as zero (never from LDS: a zero coefficient does
        // not neutralise a NaN somebody else left there).
        const int kHave = (b == 0) ? min(order, nh0) : order;
        double Y3 = 0.0, Y2 = 0.0, Y1 = 0.0;
        if (16 - m <= kHave) Y3 = y[b - 16 + m];
        if (32 - m <= kHave) Y2 = y[b - 32 + m];
        if (48 - m <= kHave) Y1 = y[b - 48 + m];
        const double z = y[b + lane];
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        asm volatile("s_nop 1" : "+v"(Y1), "+v"(Y2), "+v"(Y3));
#define VP_HC_ROW(YQ, K0) \
        VP_BI_T(acc0, YQ, R[K0 + 0], 15);  VP_BI_T(acc1, YQ, R[K0 + 1], 14);  VP_BI_T(acc2, YQ, R[K0 + 2], 13);  VP_BI_T(acc3, YQ, R[K0 + 3], 12);  \
        VP_BI_T(acc0, YQ, R[K0 + 4], 11);  VP_BI_T(acc1, YQ, R[K0 + 5], 10);  VP_BI_T(acc2, YQ, R[K0 + 6], 9);   VP_BI_T(acc3, YQ, R[K0 + 7], 8);   \
        VP_BI_T(acc0, YQ, R[K0 + 8], 7);   VP_BI_T(acc1, YQ, R[K0 + 9], 6);   VP_BI_T(acc2, YQ, R[K0 + 10], 5);  VP_BI_T(acc3, YQ, R[K0 + 11], 4);  \
        VP_BI_T(acc0, YQ, R[K0 + 12], 3);  VP_BI_T(acc1, YQ, R[K0 + 13], 2);  VP_BI_T(acc2, YQ, R[K0 + 14], 1);  VP_BI_T(acc3, YQ, R[K0 + 15], 0);
        VP_HC_ROW(Y3, 0)
        if (order > 16) { VP_HC_ROW(Y2, 16) }
        if (RN > 32 && order > 32) { VP_HC_ROW(Y1, (RN > 32 ? 32 : 0)) }
#undef VP_HC_ROW
        y[b + lane] = z + ((acc0 + acc1) + (acc2 + acc3));
    }
    STAMPG(25);
}
template <int RN = 48>
__device__ __forceinline__ void iir_block_wave_hc(const lds_f64 *x, lds_f64 *y, int n, const lds_f64 *aL, int order_, int nh0,
                                                  const lds_f64 *hpad, double gmul)
{
    iir_hc_phase1(x, y, n, hpad, gmul);
    iir_hc_phase2<RN>(y, n, aL, order_, nh0, hpad);
}

// The same decomposition for orders up to 16 in the register-light builds (two workgroups per CU, 128 VGPRs: the 64 taps of
// iir_block_wave_regs do not fit, and the LDS form spends 35 us per 1024 samples on its reads): the zero-state responses in
// four passes of 16 taps each, the history matrix row (16 entries) summed directly from the 64-sample impulse response --
// Hc[i][k] = -sum_{j=0..16-k} h[i-j] a[j+k], the coefficients through the row broadcast -- and 16 DPP terms per block in
// the serial pass.
template <int M>
__device__ __forceinline__ void fmac_row_bcast(double &acc, double rowv, double h)
{
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(rowv), "v"(h), "n"(M));
}
template <int K, int... J>
__device__ __forceinline__ double hc16_row(double arow, const double (&hl)[16], std::integer_sequence<int, J...>)
{
    double r0 = 0.0, r1 = 0.0;
    (fmac_row_bcast<J + K - 1>((J & 1) ? r1 : r0, arow, hl[J]), ...);         // -a[J + K] sits in lane J + K - 1 of the row
    return r0 + r1;
}
__device__ __forceinline__ void iir_block_wave_hc16(const lds_f64 *x, lds_f64 *y, int n, const lds_f64 *aL, int order_, int nh0,
                                                    const lds_f64 *hpad, double gmul)
{
    const int lane = vp_tid() & 63, m = lane & 15;
    const int order = __builtin_amdgcn_readfirstlane(order_);
#pragma unroll 1
    for (int q = 0; q < 4; q++) {                                             // taps 16 q .. 16 q + 15 against x[b + 16 q + ...]
        double H[16];
#pragma unroll
        for (int j = 0; j < 16; j++) H[j] = hpad[WAVE + lane - 16 * q - j];   // h[lane - 16 q - j], 0 left of the start
        for (int b = 0; b < n; b += WAVE) {
            double X0 = gmul * x[b + 16 * q + m];
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
            asm volatile("s_nop 1" : "+v"(X0));
            VP_BI_ROW(X0, 0)
            const double sum = (acc0 + acc1) + (acc2 + acc3);
            if (q == 0) y[b + lane] = sum;
            else y[b + lane] += sum;
        }
    }
    double R[16];
    {
        double hl[16];
#pragma unroll
        for (int j = 0; j < 16; j++) hl[j] = hpad[WAVE + lane - j];
        double arow = (m + 1 <= order) ? -aL[m + 1] : 0.0;
        asm volatile("s_nop 1" : "+v"(arow));
#define VP_HC16_R(K) R[K - 1] = hc16_row<K>(arow, hl, std::make_integer_sequence<int, 17 - K>{});
        VP_HC16_R(1) VP_HC16_R(2) VP_HC16_R(3) VP_HC16_R(4) VP_HC16_R(5) VP_HC16_R(6) VP_HC16_R(7) VP_HC16_R(8)
        VP_HC16_R(9) VP_HC16_R(10) VP_HC16_R(11) VP_HC16_R(12) VP_HC16_R(13) VP_HC16_R(14) VP_HC16_R(15) VP_HC16_R(16)
#undef VP_HC16_R
    }
    for (int b = 0; b < n; b += WAVE) {
        const int kHave = (b == 0) ? min(order, nh0) : order;
        double Y3 = 0.0;
        if (16 - m <= kHave) Y3 = y[b - 16 + m];          // (slots beyond the order or before the frame's start: zero, never from LDS)
        const double z = y[b + lane];
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        asm volatile("s_nop 1" : "+v"(Y3));
        VP_BI_T(acc0, Y3, R[0], 15);  VP_BI_T(acc1, Y3, R[1], 14);  VP_BI_T(acc2, Y3, R[2], 13);  VP_BI_T(acc3, Y3, R[3], 12);
        VP_BI_T(acc0, Y3, R[4], 11);  VP_BI_T(acc1, Y3, R[5], 10);  VP_BI_T(acc2, Y3, R[6], 9);   VP_BI_T(acc3, Y3, R[7], 8);
        VP_BI_T(acc0, Y3, R[8], 7);   VP_BI_T(acc1, Y3, R[9], 6);   VP_BI_T(acc2, Y3, R[10], 5);  VP_BI_T(acc3, Y3, R[11], 4);
        VP_BI_T(acc0, Y3, R[12], 3);  VP_BI_T(acc1, Y3, R[13], 2);  VP_BI_T(acc2, Y3, R[14], 1);  VP_BI_T(acc3, Y3, R[15], 0);
        y[b + lane] = z + ((acc0 + acc1) + (acc2 + acc3));
    }
}
#undef VP_BI_ROW
