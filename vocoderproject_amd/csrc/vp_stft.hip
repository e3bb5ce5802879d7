// vp_stft.hip -- the fused STFT round trip for gfx950: Hann windowing, FFT, [per-bin spectral stage], inverse FFT and overlap-add
// in ONE kernel, one frame per WAVEFRONT, the transform's butterflies in registers.
//
// NO reference counterpart (the reference contains no FFT, no STFT and no phase vocoder: SURVEY.md section 0).  These are the
// kernels BASELINE.json's north_star lists ("Hann windowing, batched FFT/iFFT, per-bin phase unwrap/accumulate and overlap-add ...
// one frame per wavefront with samples staged in LDS"); they are checked against numpy.fft and a build-authored NumPy restatement
// of the phase-vocoder stage (tests/stft_reference.py) -- parity unpinned by nature -- and reported apart from the metric.
//
// Shape of the computation (F = 1024, hop = 256; F = 128 P in general, P = complex points per lane = 8):
//   * a workgroup = VP_STFT_WAVES (4) wavefronts owns a RUN of consecutive rounds of one stream; in a round wavefront w takes frame
//     4 round + w.  Its 1024 real samples are read straight from HBM/L2 (one aligned float2 per lane and register: consecutive frames
//     overlap by 3/4, the re-reads hit L2), windowed and packed as 512 complex points z[n] = x[2n] + i x[2n+1], n = lane + 64 r.
//   * 512-point complex FFT in registers: three radix-8 steps (dft8: 56 fp64 operations on 8 points held by one lane) with two
//     exchanges through a wavefront-private 8 KB LDS buffer between them -- decimation in time in the "autosort" order, so input
//     AND output are in natural order (lane = index mod 64, register = index div 64): no bit reversal anywhere.  The exchange
//     addresses are skewed so that every ds_write_b128 / ds_read_b128 lane group hits distinct banks (tools/stft_fft_model.py
//     replays the index algebra and the bank model of MI355X_MICROARCH.md: 0 conflicts).  No barrier inside a transform: a
//     wavefront's LDS operations execute in order.
//   * real-input split: X[k] = E[k] + W^k O[k] needs Z[k] and Z[N - k]; lane j owns the pairs k = 64 q + j, q < 4, and fetches the
//     partners from lane 64 - j's upper registers (a half exchange: 4 values per lane).  The spectral stage works on the pair
//     in registers: identity (plus an optional magnitude dump) or the phase-vocoder pitch shift below.  Merge, half exchange back,
//     conjugate, the SAME forward transform again (inverse = conj FFT conj), window * 1/N * overlap-add normalisation.
//   * overlap-add in LDS, deterministic: every wavefront parks its windowed output frame (f32) in its own exchange buffer, one
//     barrier, then the workgroup adds, for every output sample of the round's hops, the frames that cover it IN FRAME ORDER onto
//     a carry of the hops the previous round left incomplete, writes each finished sample to HBM exactly once and keeps the
//     unfinished hops as the new carry.  No frame scratch in HBM, no second kernel, no atomics: HBM traffic = input once (+ L2
//     re-reads) + output once.
//   * runs: with few streams a stream is cut into runs of rounds so that the grid fills the chip; a run recomputes the
//     ceil((O - 1) / 4) rounds in front of it with stores suppressed, which rebuilds exactly the carry the previous run ends with
//     -- the additions happen in the same order, so the output does not depend on the partition (tested).
//
// Phase-vocoder stage (template PV; "per-bin phase unwrap/accumulate", north_star; the classic analysis/synthesis pitch shifter):
// per frame and bin k: magnitude and phase; phase advance against the previous frame minus the bin's nominal advance, wrapped to
// (-pi, pi] (the unwrap) -> true frequency; bins move to round(k ratio), magnitudes of bins that land together add, the frequency
// scales by the ratio; the synthesis phase accumulates the scaled advance frame after frame.  A workgroup then owns a whole
// stream (the accumulator is a recurrence over frames); inside a round the four frames' increments are summed in frame order.
#include <hip/hip_runtime.h>

#include "vp_stft.h"

#define WAVE 64
#define NWV VP_STFT_WAVES

typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) double lds_f64;
#include "vp_fft.inc"
#include "vp_fft32.inc"

// exchange buffers / output slots (8 KB per wavefront; 4 KB in the single-precision build), overlap-add carry (F - hop floats), rounded up to 16 bytes
__host__ __device__ static inline size_t stft_lds_base(int F, int hop, int f32 = 0)
{
    return (((size_t)NWV * (f32 ? 4096 : 8192) + (size_t)(F - hop) * sizeof(float)) + 15) & ~(size_t)15;
}
size_t vp_stft_lds_bytes(int F, int hop, int f32) { return stft_lds_base(F, hop, f32); }

int vp_stft_supported(int F, int hop)
{
    return (F == 1024 || F == 2048) && hop > 0 && F % hop == 0 && F / hop >= 2 && F / hop <= 16;
}

// the rounds of a workgroup's run: it stores the hops of [rFirst, r1) and recomputes [r0, rFirst) in front of them for the carry
struct StftRun { int rFirst, r0, r1; };
__device__ __forceinline__ StftRun stft_run(const VpStftArgs &A, int run)
{
    const int rFirst = run * A.roundsPerRun;
    return StftRun{rFirst, max(0, rFirst - (run > 0 ? A.haloRounds : 0)), min(rFirst + A.roundsPerRun, A.nRounds)};
}

// the samples of the 1024-point frame at x: one float2 per lane and register.  (Whether the run has the frame is the caller's test: with
// the test in here the single-precision kernel carries sixteen more moves.)
__device__ __forceinline__ void stft_load_frame(f2 (&xv)[8], const float *x, int aligned, int lane)
{
    if (aligned) {
#pragma unroll
        for (int r = 0; r < 8; r++) xv[r] = *(const f2 *)(x + 2 * (lane + 64 * r));
    } else {
#pragma unroll
        for (int r = 0; r < 8; r++) xv[r] = f2{x[2 * (lane + 64 * r)], x[2 * (lane + 64 * r) + 1]};
    }
}

// magnitude dump of one frame: |X[k]|, k <= N = 128 Q, natural order (lane 0, q = 0: X[N] sits in the mirror slot)
template <int Q, class T>
__device__ __forceinline__ void stft_mag_dump(float *m, const RPairsT<T, Q> &X, int lane)
{
    constexpr int N = 128 * Q;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const int k = 64 * q + lane;
        m[k] = (float)sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]);             // (sqrt: the float or the double overload, by T)
        m[N - k] = (float)sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]);
    }
    if (lane == 0) m[N / 2] = (float)sqrt(X.hr * X.hr + X.hi * X.hi);
}

// Overlap-add of one round, by the whole workgroup (behind the barrier that follows the wavefronts' slot writes): relative hop u of the
// round (hops rd * NWV + u) takes frames w in [u - O + 1, u] IN FRAME ORDER on top of the carry of the hops the previous round left
// incomplete; finished hops go to HBM (once), the others become the new carry.  slots: wavefront w's output frame at w * SLOT floats.
template <int SLOT = 2048>
__device__ __forceinline__ void stft_overlap_add(const VpStftArgs &A, const lds_f32 *slots, lds_f32 *carry, int s, int rd, bool emit, int tid)
{
    const int hop = A.hop, O = A.O, T = A.T;
    float *o = A.out + (size_t)s * T;
    for (int i = tid; i < hop; i += 64 * NWV) {
        for (int u = 0; u < NWV + O - 1; u++) {
            float v = (u < O - 1) ? carry[u * hop + i] : 0.f;
            const int wlo = max(0, u - O + 1), whi = min(u, NWV - 1);
            for (int w = wlo; w <= whi; w++) v += slots[w * SLOT + (u - w) * hop + i];
            if (u < NWV) {
                const long t = (long)(rd * NWV + u) * hop + i;
                if (emit && t < T) o[t] = v;
            } else carry[(u - NWV) * hop + i] = v;
        }
    }
}

#define VP_TWO_PI 6.283185307179586476925286766559

// ---- the phase-vocoder stage's elementary functions, in TURNS (round 5) -----------------------------------------------------------
// The stage kept its phases in radians and called libm: atan2 per bin, sincos of an accumulated phase of up to thousands of radians
// per bin (the device library's argument reduction for large arguments), nine of each per lane and frame -- 6000 vector instructions
// per lane and round, four fifths of the kernel's time.  In turns (1 turn = 2 pi) the reduction is a subtraction of rint(), exact, and
// what is left are three short polynomials (minimax fits on Chebyshev nodes, tools/stft_pv_fit.py; absolute errors below 4e-16 of a
// turn / of the unit circle).  Same stage, same definition (tests/stft_reference.py keeps radians and numpy's functions: an independent
// check); the outputs differ at the 1e-13 level.
__device__ static const double PV_AT[11] = {0.15915494309189532, -0.05305164769729216, 0.031830988616730685, -0.022736420283186426, 0.017683874894479496,
                                            -0.014468416126674181, 0.012238931495957754, -0.010567969142530591, 0.009050862433965945, -0.006910937165090144,
                                            0.003350241773092173};                          // atan(r) / (2 pi r) in u = r^2 on [0, tan^2(pi/8)]
__device__ static const double PV_SN[7] = {6.283185307179581, -41.341702240399435, 81.60524927567752, -76.70585960744309, 42.05867032464745, -15.092818445192446,
                                           3.7567969372293444};                              // sin(2 pi t) / t in v = t^2 on [0, 1/64]
__device__ static const double PV_CS[7] = {1.0000000000000002, -19.739208802178528, 64.93939402241888, -85.4568171016908, 60.24462112885379, -26.424298367777688,
                                           7.810833486309896};                               // cos(2 pi t) in v = t^2 on [0, 1/64]
// atan2(im, re) / (2 pi), in [-0.5, 0.5]
__device__ __forceinline__ double pv_phase_turns(double im, double re)
{
    const double ax = fabs(re), ay = fabs(im);
    const double mx = fmax(ax, ay), mn = fmin(ax, ay);
    double r = (mx > 0.0) ? mn / mx : 0.0;                                     // in [0, 1]  (atan2(0, 0) = 0)
    double base = 0.0;
    if (r > 0.41421356237309503) { r = (r - 1.0) / (r + 1.0); base = 0.125; }  // atan(r) = pi/4 + atan((r - 1) / (r + 1))
    const double u = r * r;
    double q = PV_AT[10];
#pragma unroll
    for (int i = 9; i >= 0; i--) q = __builtin_fma(q, u, PV_AT[i]);
    double t = base + q * r;                                                   // in [0, 1/8]
    if (ay > ax) t = 0.25 - t;
    if (re < 0.0) t = 0.5 - t;
    return (im < 0.0) ? -t : t;
}
// (sin, cos) of 2 pi t for any finite t
__device__ __forceinline__ void pv_sincos_turns(double t, double &sn, double &cs)
{
    t -= rint(t);                                                              // [-1/2, 1/2], exact
    const double q = rint(t * 4.0);                                            // the quarter turn, -2 .. 2
    const double r = t - q * 0.25;                                             // [-1/8, 1/8], exact
    const double v = r * r;
    double ps = PV_SN[6], pc = PV_CS[6];
#pragma unroll
    for (int i = 5; i >= 0; i--) { ps = __builtin_fma(ps, v, PV_SN[i]); pc = __builtin_fma(pc, v, PV_CS[i]); }
    const double sr = ps * r, cr = pc;
    const int iq = (int)q & 3;
    sn = (iq == 0) ? sr : (iq == 1) ? cr : (iq == 2) ? -sr : -cr;
    cs = (iq == 0) ? cr : (iq == 1) ? -sr : (iq == 2) ? -cr : sr;
}

// the workgroup's phase-vocoder work arrays (1024-point frames: VP_PV_NB bins), carved for wavefront wv
struct PvLds {
    lds_d2 *ana;               // [NWV][nb]      (magnitude, true frequency in bins) of this wavefront's frame
    lds_f64 *phPrev;           // [NWV + 1][nb]  slot w + 1: frame of wavefront w this round; slot 0: the frame before the round's first live one
    lds_f64 *inc;              // [NWV][nb]      synthesis phase increment of each wavefront's frame
    lds_f64 *sum;              // [nb]           synthesis phase accumulator in front of the round's first live frame
};
__host__ __device__ constexpr size_t pv_lds_bytes() { return (size_t)(NWV * 2 + (NWV + 1) + NWV + 1) * VP_PV_NB * sizeof(double); }
// p: 16-byte aligned (the 16-byte type comes first: nb is odd)
__device__ __forceinline__ PvLds pv_lds_carve(lds_f64 *p, int wv)
{
    constexpr int nb = VP_PV_NB;
    PvLds pv;
    pv.ana = (lds_d2 *)p + (size_t)wv * nb; p += NWV * nb * 2;
    pv.phPrev = p; p += (NWV + 1) * nb;
    pv.inc = p; p += NWV * nb;
    pv.sum = p;
    return pv;
}

// PV: phase-vocoder stage between the transforms; MAG: magnitude dump (builds of their own: the timed round trip carries neither)
template <bool PV, bool MAG>
__global__ __launch_bounds__(64 * NWV) void vp_k_stft_fused(VpStftArgs A)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 512;                                                     // complex points = F / 2
    const int F = A.F, hop = A.hop, O = A.O, T = A.T;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;                                    // this wavefront's exchange buffer ...
    lds_f32 *slots = (lds_f32 *)smem;                                          // ... whose first F floats double as its output slot (slot w at w * 2048)
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;                             // [(O - 1) hop]
    PvLds pv;
    if (PV) pv = pv_lds_carve((lds_f64 *)smem + stft_lds_base(F, hop) / 8, wv);

    // per-lane constants, once per wavefront: window values of the lane's 16 samples, transform constants, split twiddles
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
    if (PV) {
        for (int i = tid; i < VP_PV_NB; i += 64 * NWV) { pv.phPrev[i] = 0.0; pv.sum[i] = 0.0; }
    }
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * T;
    // the frame's samples are requested a round ahead (see vp_k_stft_fused32)
    f2 xv[8];
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) stft_load_frame(xv, xs + (size_t)f_ * hop, A.aligned, lane);
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        C8 z;
        RPairs X;                                                              // X[k], X[N - k] of the lane's pairs (vp_fft.inc)
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) { z.re[r] = (double)xv[r].x * wa[r].x; z.im[r] = (double)xv[r].y * wa[r].y; }
        }
        request(rd + 1);
        if (live) {
            fft512_rx(z, xb, L);
            rfft_split(z, xb, lane, (const d2 *)ws, X);
            if (MAG) stft_mag_dump<4>(A.mag + ((size_t)s * A.nFrames + f) * (N + 1), X, lane);
        }
        if (PV) {
            // ---- phase-vocoder stage, phases in TURNS.  Bins of this lane: k = 64 q + lane and N - k (q < 4); lane 0 also holds 0, N and N / 2.
            const int nb = N + 1;
            const double invO = 1.0 / (double)O;                               // nominal phase advance of bin 1 per hop, in turns (O a power of two: exact)
            const double invRatio = 1.0 / A.pvRatio;
            double ph[9];
            int kb[9];
            double mg[9];
            if (live) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    kb[2 * q] = 64 * q + lane; kb[2 * q + 1] = N - kb[2 * q];
                    mg[2 * q] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); ph[2 * q] = pv_phase_turns(X.ki[q], X.kr[q]);
                    mg[2 * q + 1] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); ph[2 * q + 1] = pv_phase_turns(X.mi[q], X.mr[q]);
                }
                kb[8] = N / 2; mg[8] = sqrt(X.hr * X.hr + X.hi * X.hi); ph[8] = pv_phase_turns(X.hi, X.hr);            // lane 0 only
#pragma unroll
                for (int e = 0; e < 9; e++) if (e < 8 || lane0) pv.phPrev[(wv + 1) * nb + kb[e]] = ph[e];
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k = kb[e];
                    double d = ph[e] - pv.phPrev[wv * nb + k] - (double)k * invO;
                    d -= rint(d);                                              // the unwrap: deviation from the nominal advance in [-1/2, 1/2] turns
                    pv.ana[k] = d2{mg[e], (double)k + d * (double)O};          // true frequency in bins
                }
                wave_sync();
                // bins move to floor(k ratio + 0.5): synthesis bin kk gathers the analysis bins that land on it, in increasing k
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int kk = kb[e];
                    const int kc = (int)((double)kk * invRatio);
                    double sm = 0.0, sf = 0.0;
                    // (the five candidates are requested at once and chosen from in registers: a conditional read per candidate was a
                    // dependent LDS round trip each, forty-five per frame -- the stage's largest single cost)
                    d2 cand[5];
#pragma unroll
                    for (int c_ = 0; c_ < 5; c_++) cand[c_] = pv.ana[min(max(kc - 2 + c_, 0), N)];
#pragma unroll
                    for (int c_ = 0; c_ < 5; c_++) {
                        const int k = kc - 2 + c_;
                        if (k >= 0 && k <= N && (int)floor((double)k * A.pvRatio + 0.5) == kk) { sm += cand[c_].x; sf = cand[c_].y * A.pvRatio; }
                    }
                    mg[e] = sm;
                    pv.inc[wv * nb + kk] = sf * invO;                           // phase advance of the synthesis bin over one hop, in turns
                }
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int kk = kb[e];
                    double sp = pv.sum[kk];
                    for (int w = 0; w <= wv; w++) sp += pv.inc[w * nb + kk];   // frames of the round in order (frames beyond the stream's last add nothing: they are never live)
                    ph[e] = sp;
                    double sn, cs;
                    pv_sincos_turns(sp, sn, cs);
                    const double re = mg[e] * cs, im = mg[e] * sn;
                    if (e == 8) { X.hr = re; X.hi = im; }
                    else if (e & 1) { X.mr[e >> 1] = re; X.mi[e >> 1] = im; }
                    else { X.kr[e >> 1] = re; X.ki[e >> 1] = im; }
                }
                if (lane0) { X.ki[0] = 0.0; X.mi[0] = 0.0; }                   // X[0], X[N] of a real frame are real: keep the real parts
            }
            __syncthreads();                                                   // every wavefront has read phPrev / sum / inc of this round
            // the last live wavefront of the round leaves the next round's "previous frame" and accumulator
            const int lastLive = min(NWV - 1, A.nFrames - 1 - rd * NWV);
            if (live && wv == lastLive) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    pv.phPrev[kb[e]] = pv.phPrev[(wv + 1) * nb + kb[e]];
                    pv.sum[kb[e]] = ph[e] - rint(ph[e]);
                }
            }
        }
        lds_f2 *slot = (lds_f2 *)(slots + wv * 2048);
        if (live) {
            // ---- merge (the inverse of the split), scaled by c = overlap-add normalisation / N, and conjugated for the inverse transform
            rfft_merge_conj(z, xb, lane, (const d2 *)ws, X, A.c);
            fft512_rx(z, xb, L);                                                  // y = FFT(conj Z'): x'[2n] = Re y, x'[2n + 1] = -Im y (1/N is in c)
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

// ---- 2048-point frames (BASELINE configs[4]'s "2048-pt FFT hop 512"): 1024 complex points, SIXTEEN per lane --------------------------
// The same round structure; the transform is a radix-2 step on top of two 512-point ones.  Forward, decimation in time: the lane loads
// z[2m] and z[2m + 1] for m = lane + 64 r (four consecutive samples: one aligned float4), E = FFT512(even), O = FFT512(odd),
// Z[k'] = E + W^k' O, Z[k' + 512] = E - W^k' O (k' = 64 q + lane: in-lane, natural order).  Backward, decimation in frequency on the
// conjugated spectrum: e = lo + hi, o = (lo - hi) W^k', two 512-point transforms, y[2k'] and y[2k' + 1] -- again four consecutive
// samples per lane and register.  The 512-point transforms' twiddles come from LDS copies of the tables (the sixteen points, the eight
// bin pairs and the top step's twiddles use the registers), the window from the global table (L1/L2-resident: 16 KB).
template <bool MAG>
__global__ __launch_bounds__(64 * NWV) void vp_k_stft_fused2k(VpStftArgs A)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 1024;                                                    // complex points = F / 2
    const int F = A.F, hop = A.hop, T = A.T;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;                                          // slot w: the whole exchange buffer (2048 floats)
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;
    lds_d2 *twL = (lds_d2 *)smem + stft_lds_base(F, hop) / 16;                 // [8][8] W_64 rows | [64][8] W_512
    FftAddr L;
    fft_addr_init(L, lane);
    for (int i = tid; i < 64; i += 64 * NWV) twL[i] = ((const d2 *)A.tw1)[(i >> 3) * 64 + (i & 7)];
    for (int i = tid; i < 512; i += 64 * NWV) twL[64 + i] = ((const d2 *)A.tw2)[i];
    const lds_d2 *tw1p = twL + (lane >> 3) * 8, *tw2p = twL + 64 + lane * 8;
    d2 wtop[8], ws[8];                                                         // W_1024^(64 q + lane), W_2048^(64 q + lane)
#pragma unroll
    for (int q = 0; q < 8; q++) { wtop[q] = ((const d2 *)A.twTop)[lane * 8 + q]; ws[q] = ((const d2 *)A.tws)[lane * 8 + q]; }
    for (int i = tid; i < F - hop; i += 64 * NWV) carry[i] = 0.f;
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * T;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) f4 lds_f4;
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;
        lds_f4 *slot = (lds_f4 *)(slots + wv * 2048);
        if (live) {
            const float *x = xs + (size_t)f * hop;
            C8 e, o;                                                           // even / odd packed points of the lane: z[2m], z[2m + 1], m = lane + 64 r
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int m = lane + 64 * r;
                f4 v;
                if (A.aligned) v = *(const f4 *)(x + 4 * m);
                else v = f4{x[4 * m], x[4 * m + 1], x[4 * m + 2], x[4 * m + 3]};
                const d2 w0 = ((const d2 *)A.win)[2 * m], w1 = ((const d2 *)A.win)[2 * m + 1];
                e.re[r] = (double)v.x * w0.x; e.im[r] = (double)v.y * w0.y;
                o.re[r] = (double)v.z * w1.x; o.im[r] = (double)v.w * w1.y;
            }
            fft512_rx(e, xb, L, tw1p, tw2p);
            fft512_rx(o, xb, L, tw1p, tw2p);
            double hr[8], hi[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {                                      // radix-2 on top: lo = E + W^k' O (kept in e), hi = E - W^k' O
                const double tr = __builtin_fma(o.re[q], wtop[q].x, -(o.im[q] * wtop[q].y)), ti = __builtin_fma(o.re[q], wtop[q].y, o.im[q] * wtop[q].x);
                hr[q] = e.re[q] - tr; hi[q] = e.im[q] - ti;
                e.re[q] += tr; e.im[q] += ti;
            }
            RPairsN<8> X;
            rfft_split_n<8>(e.re, e.im, hr, hi, xb, lane, (const d2 *)ws, X);
            if (MAG) stft_mag_dump<8>(A.mag + ((size_t)s * A.nFrames + f) * (N + 1), X, lane);
            rfft_merge_conj_n<8>(e.re, e.im, hr, hi, xb, lane, (const d2 *)ws, X, A.c);
#pragma unroll
            for (int q = 0; q < 8; q++) {                                      // radix-2 on top, decimation in frequency: e = lo + hi, o = (lo - hi) W^k'
                const double dr = e.re[q] - hr[q], di = e.im[q] - hi[q];
                e.re[q] += hr[q]; e.im[q] += hi[q];
                o.re[q] = __builtin_fma(dr, wtop[q].x, -(di * wtop[q].y)); o.im[q] = __builtin_fma(dr, wtop[q].y, di * wtop[q].x);
            }
            fft512_rx(e, xb, L, tw1p, tw2p);                                      // y[2k'] ...
            fft512_rx(o, xb, L, tw1p, tw2p);                                      // ... and y[2k' + 1], k' = lane + 64 r: x'[2n] = Re y[n], x'[2n + 1] = -Im y[n]
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int m = lane + 64 * r;
                const d2 w0 = ((const d2 *)A.win)[2 * m], w1 = ((const d2 *)A.win)[2 * m + 1];
                slot[m] = f4{(float)(e.re[r] * w0.x), (float)(-(e.im[r] * w0.y)), (float)(o.re[r] * w1.x), (float)(-(o.im[r] * w1.y))};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        stft_overlap_add(A, slots, carry, s, rd, rd >= R.rFirst, tid);
        __syncthreads();
    }
}

// ---- 2048-point frames WITH the phase-vocoder stage ------------------------------------------------------------------------------------
// vp_k_stft_fused2k's transforms, split and merge around vp_k_stft_fused<true, false>'s stage: the same definition (tests/stft_reference.py
// with F = 2048), the same operations in the same order per bin, seventeen bins per lane (k = 64 q + lane and 1024 - k, q < 8; lane 0 also
// bin 512).  The 1024 build's layout scaled to 1025 bins needs 197 KB of LDS at hop 128 and more than 512 registers; what differs here:
//   * no `inc` array.  The lane <-> bin map is the same in every wavefront, so the round's left-to-right sum sum + inc_0 + inc_1 + ... is
//     handed from wavefront to wavefront IN PLACE through `sum`: wavefront w adds its increment in its turn (a barrier between turns), keeps
//     the partial sum as its own synthesis phase, and the round's last live wavefront leaves the sum wrapped.  The additions and their
//     order are the 1024 build's.
//   * no LDS copies of the 512-point transform's twiddle tables: they, the top step's and the split's twiddles and the window come from
//     the global tables where they are used (L1 / L2-resident: 16 + 8 + 8 + 16 KB; the loads do not depend on the data and are issued
//     ahead of it).  Resident in registers the transform's twiddles are 64 more of them.
//   * nothing of the stage is carried in registers across a barrier except the gathered magnitude and increment: magnitudes and phases go
//     to the LDS arrays that hold them anyway (ana.x, phPrev) as they are computed, the bin pairs X are dead from there to the synthesis.
// LDS at hop 128: slots 32 768 + carry 7 680 + ana 65 600 + phPrev 41 000 + sum 8 200 = 155 248 B of the 163 328 B ceiling: one workgroup
// per CU, one wavefront per SIMD, hence up to 512 registers per lane.
#define VP_PV2K_NB 1025
__host__ __device__ constexpr size_t pv2k_lds_bytes() { return (size_t)(NWV * 2 + (NWV + 1) + 1) * VP_PV2K_NB * sizeof(double); }
size_t vp_stft_pv2k_lds_bytes(int hop) { return stft_lds_base(2048, hop) + pv2k_lds_bytes(); }

// bin e of the lane's seventeen: even e the pair's k = 64 (e / 2) + lane, odd e its mirror N - k, e = 16 bin N / 2 (lane 0 only)
__device__ __forceinline__ int pv2k_bin(int e, int lane) { return e == 16 ? 512 : (e & 1) ? 1024 - (64 * (e >> 1) + lane) : 64 * (e >> 1) + lane; }

__global__ __launch_bounds__(64 * NWV) void vp_k_stft_pv2k(VpStftArgs A)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 1024, nb = VP_PV2K_NB;                                   // complex points = F / 2; bins
    const int F = A.F, hop = A.hop, O = A.O, T = A.T;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;                                          // slot w: the whole exchange buffer (2048 floats)
    lds_f32 *carry = (lds_f32 *)smem + NWV * 2048;
    // the stage's arrays (the 16-byte type first: nb is odd)
    lds_d2 *ana = (lds_d2 *)smem + stft_lds_base(F, hop) / 16 + (size_t)wv * nb;   // [NWV][nb] (magnitude, true frequency in bins) of this wavefront's frame
    lds_f64 *an = (lds_f64 *)ana;
    lds_f64 *phPrev = (lds_f64 *)((lds_d2 *)smem + stft_lds_base(F, hop) / 16 + (size_t)NWV * nb);   // [NWV + 1][nb] as in PvLds
    lds_f64 *sum = phPrev + (NWV + 1) * nb;                                    // [nb] the accumulator: in front of the round, then handed through it
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)((stft_lds_base(F, hop) + pv2k_lds_bytes()) / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif
    FftAddr L;
    fft_addr_init(L, lane);
    const d2 *tw1p = (const d2 *)A.tw1 + lane * 8, *tw2p = (const d2 *)A.tw2 + lane * 8;
    const d2 *wtop = (const d2 *)A.twTop + lane * 8, *ws = (const d2 *)A.tws + lane * 8;   // W_1024^(64 q + lane), W_2048^(64 q + lane)
    const bool lane0 = lane == 0;
    for (int i = tid; i < F - hop; i += 64 * NWV) carry[i] = 0.f;
    for (int i = tid; i < nb; i += 64 * NWV) { phPrev[i] = 0.0; sum[i] = 0.0; }
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * T;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) f4 lds_f4;
    const double invO = 1.0 / (double)O;                                       // nominal phase advance of bin 1 per hop, in turns (O a power of two: exact)
    const double invRatio = 1.0 / A.pvRatio;
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;                                       // (wavefront-uniform)
        const int lastLive = min(NWV - 1, A.nFrames - 1 - rd * NWV);
        lds_f4 *slot = (lds_f4 *)(slots + wv * 2048);
        C8 e;
        double hr[8], hi[8];
        RPairsN<8> X;
        if (live) {
            const float *x = xs + (size_t)f * hop;
            C8 o;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int m = lane + 64 * r;
                f4 v;
                if (A.aligned) v = *(const f4 *)(x + 4 * m);
                else v = f4{x[4 * m], x[4 * m + 1], x[4 * m + 2], x[4 * m + 3]};
                const d2 w0 = ((const d2 *)A.win)[2 * m], w1 = ((const d2 *)A.win)[2 * m + 1];
                e.re[r] = (double)v.x * w0.x; e.im[r] = (double)v.y * w0.y;
                o.re[r] = (double)v.z * w1.x; o.im[r] = (double)v.w * w1.y;
            }
            fft512_rx(e, xb, L, tw1p, tw2p);
            fft512_rx(o, xb, L, tw1p, tw2p);
#pragma unroll
            for (int q = 0; q < 8; q++) {                                      // radix-2 on top: lo = E + W^k' O (kept in e), hi = E - W^k' O
                const d2 wt = wtop[q];
                const double tr = __builtin_fma(o.re[q], wt.x, -(o.im[q] * wt.y)), ti = __builtin_fma(o.re[q], wt.y, o.im[q] * wt.x);
                hr[q] = e.re[q] - tr; hi[q] = e.im[q] - ti;
                e.re[q] += tr; e.im[q] += ti;
            }
            rfft_split_n<8>(e.re, e.im, hr, hi, xb, lane, ws, X);
            // ---- the stage, phases in TURNS.  Magnitude and phase of the lane's bins, straight to LDS
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int k = 64 * q + lane, m = N - k;
                an[2 * k] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); phPrev[(wv + 1) * nb + k] = pv_phase_turns(X.ki[q], X.kr[q]);
                an[2 * m] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); phPrev[(wv + 1) * nb + m] = pv_phase_turns(X.mi[q], X.mr[q]);
            }
            if (lane0) { an[2 * (N / 2)] = sqrt(X.hr * X.hr + X.hi * X.hi); phPrev[(wv + 1) * nb + N / 2] = pv_phase_turns(X.hi, X.hr); }
        }
        __syncthreads();
        // The lane's bins, their candidates and the candidates' tests do not change from round to round, and hoisted out of the loop they
        // are some 200 vector and 140 scalar registers held for good (716 bytes of scratch in the first build): the stage takes its
        // lane number through a register the compiler cannot see through, and recomputes them -- a twentieth of the round's instructions.
        int ln = lane;
        asm volatile("" : "+v"(ln));
        double mg[17], sp[17];                                                 // gathered magnitude; phase increment, then synthesis phase
        if (live) {
#pragma unroll
            for (int b = 0; b < 17; b++) {
                if (b == 16 && !lane0) continue;
                const int k = pv2k_bin(b, ln);
                double d = phPrev[(wv + 1) * nb + k] - phPrev[wv * nb + k] - (double)k * invO;
                d -= rint(d);                                                  // the unwrap: deviation from the nominal advance in [-1/2, 1/2] turns
                an[2 * k + 1] = (double)k + d * (double)O;                     // true frequency in bins
            }
            wave_sync();
            // bins move to floor(k ratio + 0.5): synthesis bin kk gathers the analysis bins that land on it, in increasing k
#pragma unroll
            for (int b = 0; b < 17; b++) {
                if (b == 16 && !lane0) continue;
                const int kk = pv2k_bin(b, ln);
                const int kc = (int)((double)kk * invRatio);
                double sm = 0.0, sf = 0.0;
                d2 cand[5];
#pragma unroll
                for (int c_ = 0; c_ < 5; c_++) cand[c_] = ana[min(max(kc - 2 + c_, 0), N)];
#pragma unroll
                for (int c_ = 0; c_ < 5; c_++) {
                    const int k = kc - 2 + c_;
                    if (k >= 0 && k <= N && (int)floor((double)k * A.pvRatio + 0.5) == kk) { sm += cand[c_].x; sf = cand[c_].y * A.pvRatio; }
                }
                mg[b] = sm;
                sp[b] = sf * invO;                                             // phase advance of the synthesis bin over one hop, in turns
            }
        }
        // the round's sum in frame order, in place: wavefront w's turn comes behind the turns of the frames in front of it
#pragma unroll
        for (int w = 0; w < NWV; w++) {
            if (w > 0) __syncthreads();
            if (live && wv == w) {
#pragma unroll
                for (int b = 0; b < 17; b++) {
                    if (b == 16 && !lane0) continue;
                    const int kk = pv2k_bin(b, ln);
                    sp[b] += sum[kk];
                    sum[kk] = (w == lastLive) ? sp[b] - rint(sp[b]) : sp[b];   // the round's last live frame leaves the next round's accumulator
                }
            }
        }
        if (live) {
            // (every live wavefront is past its reads of the previous frame's phases: the turns' barriers, or program order when the
            // round's only live wavefront is wavefront 0)
            if (wv == lastLive) {
#pragma unroll
                for (int b = 0; b < 17; b++) {
                    if (b == 16 && !lane0) continue;
                    const int k = pv2k_bin(b, ln);
                    phPrev[k] = phPrev[(wv + 1) * nb + k];
                }
            }
#pragma unroll
            for (int b = 0; b < 17; b++) {
                if (b == 16 && !lane0) continue;
                double sn, cs;
                pv_sincos_turns(sp[b], sn, cs);
                const double re = mg[b] * cs, im = mg[b] * sn;
                if (b == 16) { X.hr = re; X.hi = im; }
                else if (b & 1) { X.mr[b >> 1] = re; X.mi[b >> 1] = im; }
                else { X.kr[b >> 1] = re; X.ki[b >> 1] = im; }
            }
            if (lane0) { X.ki[0] = 0.0; X.mi[0] = 0.0; }                       // X[0], X[N] of a real frame are real: keep the real parts
            // ---- merge, the radix-2 step (decimation in frequency), two transforms, window: as vp_k_stft_fused2k
            rfft_merge_conj_n<8>(e.re, e.im, hr, hi, xb, lane, ws, X, A.c);
            C8 o;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const d2 wt = wtop[q];
                const double dr = e.re[q] - hr[q], di = e.im[q] - hi[q];
                e.re[q] += hr[q]; e.im[q] += hi[q];
                o.re[q] = __builtin_fma(dr, wt.x, -(di * wt.y)); o.im[q] = __builtin_fma(dr, wt.y, di * wt.x);
            }
            fft512_rx(e, xb, L, tw1p, tw2p);                                               // y[2k'] ...
            fft512_rx(o, xb, L, tw1p, tw2p);                                               // ... and y[2k' + 1], k' = lane + 64 r: x'[2n] = Re y[n], x'[2n + 1] = -Im y[n]
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int m = lane + 64 * r;
                const d2 w0 = ((const d2 *)A.win)[2 * m], w1 = ((const d2 *)A.win)[2 * m + 1];
                slot[m] = f4{(float)(e.re[r] * w0.x), (float)(-(e.im[r] * w0.y)), (float)(o.re[r] * w1.x), (float)(-(o.im[r] * w1.y))};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        stft_overlap_add(A, slots, carry, s, rd, rd >= R.rFirst, tid);
        __syncthreads();
    }
}

// ---- single precision (vp_stft_set_precision(t, VP_STFT_F32); 1024-point frames) ------------------------------------------------------
// The same kernel with the transform, split and merge in f32 (vp_fft32.inc).  Why it is a build of its own and not the default: the fp64
// kernel is bound by its instruction stream -- 613 fp64 vector instructions per lane and frame at 4 cycles each, two wavefronts per SIMD
// (223 registers) -- and an f32 vector instruction issues in 2 cycles once two wavefronts share the SIMD (MI355X_MICROARCH.md,
// "vector-instruction ISSUE cost"); it also needs half the registers (four wavefronts per SIMD instead of two) and half the LDS
// bytes per exchange.  The input is f32 and the output is f32 either way; what changes is the rounding inside: ~1e-7 relative per
// frame instead of ~1e-16, two orders below the 1e-4 the north_star allows -- but not the bit pattern of the default build, hence opt-in.
template <bool MAG>
__global__ __launch_bounds__(64 * NWV, 4) void vp_k_stft_fused32(VpStftArgs A)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 512;
    const int F = A.F, hop = A.hop, T = A.T;
    lds_f2 *xb = (lds_f2 *)smem + wv * 512;                                    // the wavefront's exchange buffer (4 KB) = its output slot (F floats)
    lds_f32 *slots = (lds_f32 *)smem;
    lds_f32 *carry = (lds_f32 *)smem + NWV * 1024;
    Fft32Addr L;
    fft32_addr_init(L, lane);
    // the double-precision tables, rounded once: the second step's twiddles (a row of eight per lane >> 3: 64 values) in LDS, the rest in registers
    lds_f2 *tw1L = (lds_f2 *)((lds_f32 *)smem + stft_lds_base(F, hop, 1) / 4);
    if (tid < 64) { const d2 t = ((const d2 *)A.tw1)[(tid >> 3) * 64 + (tid & 7)]; tw1L[tid] = f2{(float)t.x, (float)t.y}; }
    const lds_f2 *tw1 = tw1L + (lane >> 3) * 8;
    f2 tw2[8], wa[8], ws[4];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const d2 t2 = ((const d2 *)A.tw2)[lane * 8 + r], w = ((const d2 *)A.win)[lane + 64 * r];
        tw2[r] = f2{(float)t2.x, (float)t2.y}; wa[r] = f2{(float)w.x, (float)w.y};
    }
#pragma unroll
    for (int q = 0; q < 4; q++) { const d2 t = ((const d2 *)A.tws)[lane * 4 + q]; ws[q] = f2{(float)t.x, (float)t.y}; }
    const float c = (float)A.c;
    for (int i = tid; i < F - hop; i += 64 * NWV) carry[i] = 0.f;
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * T;
    // the frame's samples are requested a round ahead (16 registers this build can afford; +3 to +8 % on one box: 570 -> 590 M frames/s at
    // 256 streams x 65 536 samples, 675 -> 730 M at 4096 x 32 768)
    f2 xv[8];
    auto request = [&](int rd_) {
        const int f_ = rd_ * NWV + wv;
        if (rd_ < R.r1 && f_ < A.nFrames) stft_load_frame(xv, xs + (size_t)f_ * hop, A.aligned, lane);
    };
    request(R.r0);
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;
        C8f z;
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; r++) { z.re[r] = xv[r].x * wa[r].x; z.im[r] = xv[r].y * wa[r].y; }
        }
        request(rd + 1);
        if (live) {
            fft512f(z, xb, L, tw1, (const f2 *)tw2);
            RPairsT<float, 4> X;
            rfft_split_n<4>(z.re, z.im, z.re + 4, z.im + 4, xb, lane, (const f2 *)ws, X);
            if (MAG) stft_mag_dump<4>(A.mag + ((size_t)s * A.nFrames + f) * (N + 1), X, lane);
            rfft_merge_conj_n<4>(z.re, z.im, z.re + 4, z.im + 4, xb, lane, (const f2 *)ws, X, c);
            fft512f(z, xb, L, tw1, (const f2 *)tw2);
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) lds_put(xb, lane + 64 * r, z.re[r] * wa[r].x, -(z.im[r] * wa[r].y));
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) xb[lane + 64 * r] = f2{0.f, 0.f};
        }
        __syncthreads();
        stft_overlap_add<1024>(A, slots, carry, s, rd, rd >= R.rFirst, tid);
        __syncthreads();
    }
}

// single precision, 2048-point frames: vp_k_stft_fused2k's radix-2 step over two 512-point transforms, in f32.  The wavefront's output slot
// (8 KB) starts with its exchange buffer (4 KB); the window (f32, 8 KB) and the second step's twiddle rows are LDS copies: 47 KB per
// workgroup, three workgroups per CU.
template <bool MAG>
__global__ __launch_bounds__(64 * NWV, 3) void vp_k_stft_fused2k32(VpStftArgs A)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y, run = blockIdx.x;
    constexpr int N = 1024;
    const int F = A.F, hop = A.hop, T = A.T;
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) f4 lds_f4;
    lds_f32 *slots = (lds_f32 *)smem;                                          // slot w: 2048 floats at w * 2048
    lds_f32 *carry = slots + NWV * 2048;
    lds_f2 *xb = (lds_f2 *)(slots + wv * 2048);
    lds_f4 *winL = (lds_f4 *)((lds_f32 *)smem + stft_lds_base(F, hop, 0) / 4);              // [512] the window, four consecutive samples per entry
    lds_f2 *twL = (lds_f2 *)(winL + 512);                                                    // [8][8] W_64 rows (| [64][8] W_512 in the magnitude-dump build)
    Fft32Addr L;
    fft32_addr_init(L, lane);
    for (int i = tid; i < 64; i += 64 * NWV) { const d2 t = ((const d2 *)A.tw1)[(i >> 3) * 64 + (i & 7)]; twL[i] = f2{(float)t.x, (float)t.y}; }
    const lds_f2 *tw1p = twL + (lane >> 3) * 8;
    for (int i = tid; i < 512; i += 64 * NWV) {
        const d2 w0 = ((const d2 *)A.win)[2 * i], w1 = ((const d2 *)A.win)[2 * i + 1];
        winL[i] = f4{(float)w0.x, (float)w0.y, (float)w1.x, (float)w1.y};
    }
    // the third step's twiddles are the lane's own: registers (the magnitude-dump build, which is not the timed one, has none to spare
    // and reads them from an LDS copy)
    f2 wtop[8], ws[8], tw2r[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const d2 t = ((const d2 *)A.twTop)[lane * 8 + q], u = ((const d2 *)A.tws)[lane * 8 + q], v = ((const d2 *)A.tw2)[lane * 8 + q];
        wtop[q] = f2{(float)t.x, (float)t.y}; ws[q] = f2{(float)u.x, (float)u.y};
        if (MAG) twL[64 + lane * 8 + q] = f2{(float)v.x, (float)v.y}; else tw2r[q] = f2{(float)v.x, (float)v.y};
    }
    auto fft = [&](C8f &z_) {
        if (MAG) fft512f(z_, xb, L, tw1p, (const lds_f2 *)(twL + 64 + lane * 8)); else fft512f(z_, xb, L, tw1p, (const f2 *)tw2r);
    };
    const float c = (float)A.c;
    for (int i = tid; i < F - hop; i += 64 * NWV) carry[i] = 0.f;
    __syncthreads();

    const StftRun R = stft_run(A, run);
    const float *xs = A.in + (size_t)s * T;
    for (int rd = R.r0; rd < R.r1; rd++) {
        const int f = rd * NWV + wv;
        const bool live = f < A.nFrames;
        lds_f4 *slot = (lds_f4 *)(slots + wv * 2048);
        if (live) {
            const float *x = xs + (size_t)f * hop;
            C8f e, o;
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int m = lane + 64 * r;
                f4 v;
                if (A.aligned) v = *(const f4 *)(x + 4 * m);
                else v = f4{x[4 * m], x[4 * m + 1], x[4 * m + 2], x[4 * m + 3]};
                const f4 w = winL[m];
                e.re[r] = v.x * w.x; e.im[r] = v.y * w.y;
                o.re[r] = v.z * w.z; o.im[r] = v.w * w.w;
            }
            fft(e);
            fft(o);
            float hr[8], hi[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const float tr = vp_fma(o.re[q], wtop[q].x, -(o.im[q] * wtop[q].y)), ti = vp_fma(o.re[q], wtop[q].y, o.im[q] * wtop[q].x);
                hr[q] = e.re[q] - tr; hi[q] = e.im[q] - ti;
                e.re[q] += tr; e.im[q] += ti;
            }
            RPairsT<float, 8> X;
            rfft_split_n<8>(e.re, e.im, hr, hi, xb, lane, (const f2 *)ws, X);
            if (MAG) stft_mag_dump<8>(A.mag + ((size_t)s * A.nFrames + f) * (N + 1), X, lane);
            rfft_merge_conj_n<8>(e.re, e.im, hr, hi, xb, lane, (const f2 *)ws, X, c);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const float dr = e.re[q] - hr[q], di = e.im[q] - hi[q];
                e.re[q] += hr[q]; e.im[q] += hi[q];
                o.re[q] = vp_fma(dr, wtop[q].x, -(di * wtop[q].y)); o.im[q] = vp_fma(dr, wtop[q].y, di * wtop[q].x);
            }
            fft(e);
            fft(o);
            wave_sync();                                                       // (the slot starts with the exchange buffer)
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const f4 w = winL[lane + 64 * r];
                slot[lane + 64 * r] = f4{e.re[r] * w.x, -(e.im[r] * w.y), o.re[r] * w.z, -(o.im[r] * w.w)};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; r++) slot[lane + 64 * r] = f4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        stft_overlap_add(A, slots, carry, s, rd, rd >= R.rFirst, tid);
        __syncthreads();
    }
}

// hipFuncSetAttribute acts on the CURRENT device: every handle raises the two phase-vocoder builds' dynamic-LDS ceiling on its own device
// at create (vp_stft_create, behind hipSetDevice), and a failure is the caller's VP_ERR_HIP -- not a process-wide flag set once.
hipError_t vp_stft_prepare_device()
{
    const hipError_t e = hipFuncSetAttribute((const void *)vp_k_stft_fused<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)vp_k_stft_pv2k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_stft_launch(const VpStftArgs &a, int nStreams, int nRuns, hipStream_t st)
{
    const size_t lds = vp_stft_lds_bytes(a.F, a.hop, a.f32);
    const dim3 grid(nRuns, nStreams), block(64 * NWV);
    if (a.f32 && a.F == 2048) {
        // slots + carry as in the double-precision build, then the f32 copies of the window and of the second step's twiddle rows
        const size_t lds2k = vp_stft_lds_bytes(a.F, a.hop, 0) + 2048 * 4 + 64 * 8;
        if (a.mag) hipLaunchKernelGGL((vp_k_stft_fused2k32<true>), grid, block, lds2k + 512 * 8, st, a);
        else hipLaunchKernelGGL((vp_k_stft_fused2k32<false>), grid, block, lds2k, st, a);
    } else if (a.f32) {
        const size_t lds32 = lds + 64 * 8;                                      // + the second step's twiddle rows
        if (a.mag) hipLaunchKernelGGL((vp_k_stft_fused32<true>), grid, block, lds32, st, a);
        else hipLaunchKernelGGL((vp_k_stft_fused32<false>), grid, block, lds32, st, a);
    } else if (a.pv && a.F == 2048) {
        hipLaunchKernelGGL(vp_k_stft_pv2k, grid, block, lds + pv2k_lds_bytes(), st, a);       // (before the plain 2048 branch, which has no stage)
    } else if (a.F == 2048) {
        const size_t lds2 = lds + (64 + 512) * 16;                             // + the LDS copies of the 512-point transform's twiddle tables
        if (a.mag) hipLaunchKernelGGL((vp_k_stft_fused2k<true>), grid, block, lds2, st, a);
        else hipLaunchKernelGGL((vp_k_stft_fused2k<false>), grid, block, lds2, st, a);
    } else if (a.pv)
        hipLaunchKernelGGL((vp_k_stft_fused<true, false>), grid, block, lds + pv_lds_bytes(), st, a);
    else if (a.mag)
        hipLaunchKernelGGL((vp_k_stft_fused<false, true>), grid, block, lds, st, a);
    else
        hipLaunchKernelGGL((vp_k_stft_fused<false, false>), grid, block, lds, st, a);
    return hipGetLastError();
}

// ---- streaming phase vocoder (vp_pv_*, include/vp_amd.h) ---------------------------------------------------------------------------
// vp_k_stft_fused<true, false> block by block: one workgroup per stream and call, the stream's state in HBM between calls (VpPvArgs).
// Frame f of the stream covers samples [f hop, f hop + F) of everything it received since create / reset and is computed in the call in
// which its last sample arrives; wavefront w takes the frames 4 r + w by their global index, so the rounds of four frames are the
// one-shot's, cut where the calls cut them.  The stage below is the one-shot's, statement for statement (same operations on the same
// operands: the outputs agree bit for bit; ONE force-inlined function for both kernels compiles to another instruction mix and cost the
// one-shot 2 %: docs/HISTORY.md), except for what a round cut by a call needs:
//   * the first live frame of the call reads its "previous frame" phases from slot 0 (the state), whatever its wavefront;
//   * the accumulator of a round sums from the first live frame; a round that the call ends early leaves its partial sum UNWRAPPED (the
//     next call continues the same left-to-right sum) and only a round's frame 4 r + 3 wraps it;
//   * the overlap-add works on a ring of one-shot samples (VP_PV_RING floats): frames add in frame order onto what earlier frames and
//     calls left (every sample starts from 0.f, as in stft_overlap_add), and a sample leaves the ring, to output time t + L, once the
//     frames that cover it are all in and t + L falls inside the call.  Ring word q belongs to thread q mod 256 throughout: no barrier
//     between a round's additions and its stores.
// History (samples of frames not yet complete, < F), carry (< F unfinished or unemitted samples), phases, accumulator, ratio and the
// sample counter are read into LDS at entry and written back at exit.
// What of this is the arithmetic of one process call and not signal processing -- which frames complete in the call, history and carry
// between the record and LDS, the slab index maps, the ring's overlap-add and emission, the flush -- is the pv_call_* helpers below, ONE
// copy for four of the seven streaming kernels: this one, vp_k_pv_stream_lockf, vp_k_hz_stream and vp_k_xs_stream.  The kernels keep
// their LDS carve, per-lane constants, request prefetch, stage, merge and their own record fields.  vp_k_pv_stream_curve, _lock and
// _formant keep the same statements WRITTEN OUT: through the helpers they ran 0.6 - 1.2 % slower (docs/HISTORY.md).
// LDS: exchange buffers / output slots, ring, history, then the one-shot's phase-vocoder arrays (124 KB: one workgroup per CU)
__host__ __device__ constexpr size_t pv_stream_lds_bytes() { return (size_t)NWV * 8192 + (VP_PV_RING + 1024) * sizeof(float) + pv_lds_bytes(); }

// the call's interval changes and resets that concern stream s, in the order they were made (arguments: scalar, uniform): the last new
// ratio replaces `ratio`; returns whether the stream was reset
__device__ __forceinline__ bool pv_scan_updates(const VpPvArgs &A, int s, double &ratio)
{
    bool rst = false;
    for (int i = 0; i < A.nUpd; i++) {
        if (A.upd[i].stream != s && A.upd[i].stream != -1) continue;
        if (A.upd[i].ratio > 0.0) ratio = A.upd[i].ratio;
        if (A.upd[i].reset) rst = true;
    }
    return rst;
}

// ---- one process call's bookkeeping (F = 1024, four wavefronts) ----
// A stream that has received n samples takes M more.  Indices are RELATIVE to sample fa hop, the start of the first frame the call
// completes: the history is [0, H), the call's samples [H, H + M), relative frame fr covers [fr hop, fr hop + F).
struct PvCall {
    int M;                      // samples this call
    long long R;                // samples received after it
    long long fa;               // frames complete before the call (fa + nf after it)
    int nf;                     // frames of this call
    int H;                      // history: samples [fa hop, n) (< F)
    int er;                     // relative index of the next sample to emit (output time n)
    int fr0;                    // relative frame of wavefront 0 in the first round (<= 0: wavefront w takes the frames 4 r + w by global index)
};
constexpr int PV_CALL_F = 1024, PV_CALL_RM = VP_PV_RING - 1, PV_CALL_T = 64 * NWV;

__host__ __device__ constexpr PvCall pv_call_geometry(long long n, int M, int hop, int L)
{
    const long long R = n + M;
    const long long fa = n >= PV_CALL_F ? (n - PV_CALL_F) / hop + 1 : 0;
    const long long fb = R >= PV_CALL_F ? (R - PV_CALL_F) / hop + 1 : 0;
    const int nf = (int)(fb - fa);
    const int H = (int)(n - fa * hop);
    return PvCall{M, R, fa, nf, H, H - L, -(int)(fa & 3)};
}
// the call's rounds of four frames.  A function of its own, called where the kernels' round loops begin: as a member filled by
// pv_call_geometry (in front of the state loads) a kernel built on it took 6 more registers (docs/HISTORY.md)
__host__ __device__ constexpr int pv_call_rounds(const PvCall &c) { return c.nf > 0 ? (c.nf - c.fr0 + NWV - 1) / NWV : 0; }
constexpr bool pv_call_is(const PvCall &c, long long fa, long long fb, int nf, int H, int er, int fr0, int nRounds)
{
    return c.fa == fa && c.fa + c.nf == fb && c.nf == nf && c.H == H && c.er == er && c.fr0 == fr0 && pv_call_rounds(c) == nRounds;
}
//                                          n     M  hop     L    fa  fb  nf    H    er fr0 nRounds
static_assert(pv_call_is(pv_call_geometry(0, 64, 256, 960), 0, 0, 0, 0, -960, 0, 0), "a first call in which no frame completes");
static_assert(pv_call_is(pv_call_geometry(0, 1024, 256, 768), 0, 1, 1, 0, -768, 0, 1), "the stream's first frame");
static_assert(pv_call_is(pv_call_geometry(1024, 256, 256, 768), 1, 2, 1, 768, 0, -1, 1), "a call whose first frame is wavefront 1's");
static_assert(pv_call_is(pv_call_geometry(1792, 4096, 256, 768), 4, 20, 16, 768, 0, 0, 4), "four whole rounds");
// hop 128, three blocks of 100 (L = 1024 - gcd(100, 128)): fa = 76 / 128 + 1, fb = 376 / 128 + 1, H = 1100 - 128, rounds = (2 + 1 + 3) / 4
static_assert(pv_call_is(pv_call_geometry(1100, 300, 128, 1020), 1, 3, 2, 972, -48, -1, 1), "hop 128, N no multiple of the hop");

// state -> LDS.  The history; then the ring from the carry, carry[i] = one-shot sample er + i (a reset stream starts from zeros)
__device__ __forceinline__ void pv_call_load_hist(const PvCall &c, lds_f32 *hist, const float *recHist, int tid)
{
    for (int i = tid; i < c.H; i += PV_CALL_T) hist[i] = recHist[i];
}
__device__ __forceinline__ void pv_call_load_ring(const PvCall &c, lds_f32 *ring, const float *recCarry, bool rst, int tid)
{
    for (int q = tid; q < VP_PV_RING; q += PV_CALL_T) {
        const int i = (q - c.er) & PV_CALL_RM;
        ring[q] = (i < PV_CALL_F && !rst) ? recCarry[i] : 0.f;
    }
}

// the index maps over [block][stream][NB] slabs; xs / ys point at stream s of block 0
// sample at relative index rel (>= 0): the history below H, this call's blocks above
__device__ __forceinline__ float pv_call_sample(const PvCall &c, const lds_f32 *hist, const float *xs, int NB, int S, int rel)
{
    if (rel < c.H) return hist[rel];
    const unsigned k = (unsigned)(rel - c.H), b = k / (unsigned)NB;
    return xs[(size_t)b * S * NB + (k - b * NB)];
}
// the finished ring samples of relative indices [from, to) leave to output time n + (j - er), j - er in [0, M); ring word q belongs to
// thread q mod 256 throughout: no barrier between a round's additions and its stores
__device__ __forceinline__ void pv_call_emit(const PvCall &c, lds_f32 *ring, float *ys, int NB, int S, int from, int to, int tid)
{
    for (int j = from + ((tid - from) & (PV_CALL_T - 1)); j < to; j += PV_CALL_T) {
        const float v = ring[j & PV_CALL_RM];
        const unsigned k = (unsigned)(j - c.er), b = k / (unsigned)NB;
        ys[(size_t)b * S * NB + (k - b * NB)] = v;
        ring[j & PV_CALL_RM] = 0.f;
    }
}

// a round's tail (between the barrier behind the slot writes and the round's last): the overlap-add of the round's frames
// [frW0 + wFirst, frW0 + wLast] in frame order, then the samples they finish that fall inside the call.  Returns the next relative index to
// emit (uniform).  After the last round pv_call_emit(c, .., cb, c.er + c.M, ..) flushes the rest of the call's output: finished in earlier
// calls or rounds (or before the stream's first sample: zeros)
__device__ __forceinline__ int pv_call_round_tail(const PvCall &c, lds_f32 *ring, const lds_f32 *slots, float *ys, int NB, int S, int hop, int frW0, int wFirst,
                                                  int wLast, int cb, int tid)
{
    const int frA = frW0 + wFirst, frB = frW0 + wLast;
    const int lo = frA * hop, hi = frB * hop + PV_CALL_F;
    for (int j = lo + ((tid - lo) & (PV_CALL_T - 1)); j < hi; j += PV_CALL_T) {
        float v = ring[j & PV_CALL_RM];
        for (int w = wFirst; w <= wLast; w++) {
            const int o = j - (frW0 + w) * hop;
            if (o >= 0 && o < PV_CALL_F) v += slots[w * 2048 + o];
        }
        ring[j & PV_CALL_RM] = v;
    }
    const int emitEnd = min((frB + 1) * hop, c.er + c.M);
    pv_call_emit(c, ring, ys, NB, S, cb, emitEnd, tid);
    return max(cb, emitEnd);
}

// LDS -> state.  History: samples [fb hop, R); carry: one-shot samples from the next one to emit (relative er + M) on
__device__ __forceinline__ void pv_call_store_hist(const PvCall &c, float *recHist, const lds_f32 *hist, const float *xs, int NB, int S, int hop, int tid)
{
    const int Hn = c.H + c.M - c.nf * hop;
    for (int i = tid; i < Hn; i += PV_CALL_T) recHist[i] = pv_call_sample(c, hist, xs, NB, S, c.nf * hop + i);
}
__device__ __forceinline__ void pv_call_store_carry(const PvCall &c, float *recCarry, const lds_f32 *ring, int tid)
{
    const int ern = c.er + c.M;
    for (int q = tid; q < VP_PV_RING; q += PV_CALL_T) {
        const int i = (q - ern) & PV_CALL_RM;
        if (i < PV_CALL_F) recCarry[i] = ring[q];
    }
}

__global__ __launch_bounds__(64 * NWV) void vp_k_pv_stream(VpPvArgs A)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x;
    constexpr int N = 512, F = 1024, nb = N + 1;
    const int hop = A.hop, O = A.O, NB = A.N, S = A.S;
    lds_d2 *xb = (lds_d2 *)smem + wv * 512;
    lds_f32 *slots = (lds_f32 *)smem;                                          // wavefront w's output frame at w * 2048
    lds_f32 *ring = (lds_f32 *)smem + NWV * 2048;                              // [VP_PV_RING]
    lds_f32 *hist = ring + VP_PV_RING;                                         // [F]
    const PvLds pv = pv_lds_carve((lds_f64 *)(hist + F), wv);
#ifdef VP_POISON_LDS
    for (int i = tid; i < (int)(pv_stream_lds_bytes() / 8); i += 64 * NWV) ((lds_f64 *)smem)[i] = __builtin_nan("0x5a5a");
    __syncthreads();
#endif
    unsigned char *rec = A.state + (size_t)s * VP_PV_REC_BYTES;
    double *recD = (double *)rec;
    float *recHist = (float *)(rec + VP_PV_HIST_BYTES), *recCarry = (float *)(rec + VP_PV_CARRY_BYTES);

    double ratio = recD[VP_PV_RATIO];
    long long n = ((const long long *)recD)[VP_PV_COUNT];                     // samples received before this call
    const bool rst = pv_scan_updates(A, s, ratio);
    if (rst) n = 0;
    const PvCall C = pv_call_geometry(n, A.nBlocks * NB, hop, A.L);
    const int nf = C.nf;

    // state -> LDS (a reset stream starts from zeros)
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
    int cb = C.er;                                                             // next relative index to emit (uniform)
    f2 xv[8];
    auto request = [&](int k_) {
        const int fr_ = C.fr0 + NWV * k_ + wv;
        if (k_ < nRounds && fr_ >= 0 && fr_ < nf) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int rel = fr_ * hop + 2 * (lane + 64 * r);
                xv[r] = f2{pv_call_sample(C, hist, xs, NB, S, rel), pv_call_sample(C, hist, xs, NB, S, rel + 1)};
            }
        }
    };
    request(0);
    for (int k = 0; k < nRounds; k++) {
        const int frW0 = C.fr0 + NWV * k;                                      // relative frame of wavefront 0 in this round
        const int fr = frW0 + wv;
        const bool live = fr >= 0 && fr < nf;                                  // (wavefront-uniform)
        const int wFirst = max(0, -frW0), wLast = min(NWV - 1, nf - 1 - frW0);
        C8 z;
        RPairs X;
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
            const double invO = 1.0 / (double)O;
            const double invRatio = 1.0 / ratio;
            const int prevSlot = wv == wFirst ? 0 : wv;                        // the call's first frame continues from the state
            double ph[9];
            int kb[9];
            double mg[9];
            if (live) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    kb[2 * q] = 64 * q + lane; kb[2 * q + 1] = N - kb[2 * q];
                    mg[2 * q] = sqrt(X.kr[q] * X.kr[q] + X.ki[q] * X.ki[q]); ph[2 * q] = pv_phase_turns(X.ki[q], X.kr[q]);
                    mg[2 * q + 1] = sqrt(X.mr[q] * X.mr[q] + X.mi[q] * X.mi[q]); ph[2 * q + 1] = pv_phase_turns(X.mi[q], X.mr[q]);
                }
                kb[8] = N / 2; mg[8] = sqrt(X.hr * X.hr + X.hi * X.hi); ph[8] = pv_phase_turns(X.hi, X.hr);
#pragma unroll
                for (int e = 0; e < 9; e++) if (e < 8 || lane0) pv.phPrev[(wv + 1) * nb + kb[e]] = ph[e];
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int k_ = kb[e];
                    double d = ph[e] - pv.phPrev[prevSlot * nb + k_] - (double)k_ * invO;
                    d -= rint(d);
                    pv.ana[k_] = d2{mg[e], (double)k_ + d * (double)O};
                }
                wave_sync();
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int kk = kb[e];
                    const int kc = (int)((double)kk * invRatio);
                    double sm = 0.0, sf = 0.0;
                    d2 cand[5];
#pragma unroll
                    for (int c_ = 0; c_ < 5; c_++) cand[c_] = pv.ana[min(max(kc - 2 + c_, 0), N)];
#pragma unroll
                    for (int c_ = 0; c_ < 5; c_++) {
                        const int k_ = kc - 2 + c_;
                        if (k_ >= 0 && k_ <= N && (int)floor((double)k_ * ratio + 0.5) == kk) { sm += cand[c_].x; sf = cand[c_].y * ratio; }
                    }
                    mg[e] = sm;
                    pv.inc[wv * nb + kk] = sf * invO;
                }
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    const int kk = kb[e];
                    double sp = pv.sum[kk];
                    for (int w = wFirst; w <= wv; w++) sp += pv.inc[w * nb + kk];
                    ph[e] = sp;
                    double sn, cs;
                    pv_sincos_turns(sp, sn, cs);
                    const double re = mg[e] * cs, im = mg[e] * sn;
                    if (e == 8) { X.hr = re; X.hi = im; }
                    else if (e & 1) { X.mr[e >> 1] = re; X.mi[e >> 1] = im; }
                    else { X.kr[e >> 1] = re; X.ki[e >> 1] = im; }
                }
                if (lane0) { X.ki[0] = 0.0; X.mi[0] = 0.0; }
            }
            __syncthreads();
            // the round's last live frame leaves the phases and the accumulator: wrapped at a round's end, the partial sum otherwise
            if (live && wv == wLast) {
#pragma unroll
                for (int e = 0; e < 9; e++) {
                    if (e == 8 && !lane0) continue;
                    pv.phPrev[kb[e]] = pv.phPrev[(wv + 1) * nb + kb[e]];
                    pv.sum[kb[e]] = wv == NWV - 1 ? ph[e] - rint(ph[e]) : ph[e];
                }
            }
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

    // LDS -> state
    pv_call_store_hist(C, recHist, hist, xs, NB, S, hop, tid);
    pv_call_store_carry(C, recCarry, ring, tid);
    __syncthreads();                                                           // (slot 0 / sum of the last round)
    for (int i = tid; i < nb; i += 64 * NWV) { recD[i] = pv.phPrev[i]; recD[nb + i] = pv.sum[i]; }
    if (tid == 0) { recD[VP_PV_RATIO] = ratio; ((long long *)recD)[VP_PV_COUNT] = C.R; }
}

// the updates alone (a call with more than VP_PV_MAX_UPDATES of them pending enqueues this first, on the same stream)
__global__ __launch_bounds__(256) void vp_k_pv_update(VpPvArgs A)
{
    const int s = blockIdx.x;
    unsigned char *rec = A.state + (size_t)s * VP_PV_REC_BYTES;
    double *recD = (double *)rec;
    double ratio = 0.0;
    const bool rst = pv_scan_updates(A, s, ratio);
    if (rst) {
        float *recCarry = (float *)(rec + VP_PV_CARRY_BYTES);
        for (int i = threadIdx.x; i < VP_PV_NB; i += 256) { recD[i] = 0.0; recD[VP_PV_NB + i] = 0.0; }
        for (int i = threadIdx.x; i < 1024; i += 256) recCarry[i] = 0.f;
        if (threadIdx.x == 0) ((long long *)recD)[VP_PV_COUNT] = 0;
    }
    if (threadIdx.x == 0 && ratio > 0.0) recD[VP_PV_RATIO] = ratio;
}

size_t vp_pv_lds_bytes() { return pv_stream_lds_bytes(); }

hipError_t vp_pv_prepare_device()
{
    return hipFuncSetAttribute((const void *)vp_k_pv_stream, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
}

hipError_t vp_pv_launch(const VpPvArgs &a, hipStream_t st)
{
    if (a.nBlocks == 0) hipLaunchKernelGGL(vp_k_pv_update, dim3(a.S), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(vp_k_pv_stream, dim3(a.S), dim3(64 * NWV), vp_pv_lds_bytes(), st, a);
    return hipGetLastError();
}

// ---- the parts: every derived kernel family is a file of its own, included here and nowhere else.  All of them use this file's helpers,
// tables and carves; a part stands behind the parts named in its brackets, whose helpers it uses.  (tests/test_stft_parts_cpu.py holds
// the same list, in the same order.)
//   curve          vp_stft_pitch_shift_curve, vp_pv_process_blocks_curve_device: the kernels along a per-frame / per-block ratio curve
//   stretch        vp_stft_time_stretch: frames analysed at caller-given positions
//   lock           vp_stft_pitch_shift_locked, vp_pv_process_blocks_locked_device: the curve kernels with peak locking [curve: pv_curve_clamp]
//   lockf          vp_stft_pitch_shift_locked_subbin, vp_pv_process_blocks_locked_subbin_device: the locked kernels with sub-bin region
//                  offsets [curve: pv_curve_clamp; lock: its carve and sizes, pv_lock_mask, pv_lock_nearest, pv_lock_bin, pv_lock_turn]
//   harm           vp_stft_harmonize, vp_hz_process_blocks_device: several locked voices and the dry signal from one analysis
//                  [curve: pv_curve_clamp; lock: its carve and sizes, pv_lock_mask, pv_lock_nearest, pv_lock_bin]
//   stretch_lock   vp_stft_time_stretch_locked: the locked kernel with frames at caller-given positions [curve: pv_curve_clamp; stretch:
//                  pv_stretch_frame; lock: its carve and sizes, masks, pv_lock_turn, pv_lock_gather]
//   cross          vp_stft_cross_synth, vp_xs_process_blocks_device: the voice's spectral envelope on the carrier [none]
//   onset          vp_stft_onset_flux: the rectified flux and mass of the input's own frame grid, the transient-preserving stretch's first
//                  half [none]; the host half (picking the onsets, planning the positions) is vp_onset_host.inc, included by vp_capi.hip
//   stretch_reset  vp_stft_time_stretch_locked_reset: the locked stretch with a phase reset on flagged frames, its second half
//                  [stretch_lock: pv_stretch_lock_plan; and what that part stands behind]
//   formant        vp_stft_pitch_shift_formant, vp_pv_process_blocks_formant_device: the curve kernels with the cepstral formant
//                  correction [curve: pv_curve_clamp]
#include "vp_stft_curve.inc"
#include "vp_stft_stretch.inc"
#include "vp_stft_lock.inc"
#include "vp_stft_lockf.inc"
#include "vp_stft_harm.inc"
#include "vp_stft_stretch_lock.inc"
#include "vp_stft_cross.inc"
#include "vp_stft_onset.inc"
#include "vp_stft_stretch_reset.inc"
#include "vp_stft_formant.inc"
