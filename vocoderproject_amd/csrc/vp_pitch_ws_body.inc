// ------------------------------------------------------------------------------------------------
// The kernel body: prologue (everything the block needs from HBM in one round trip, as in pitch_kernel_body: MyBuffer::fillInputBuffers
// MyBuffer.cpp:74-105, the whole-ring gate :258-261, the tracker state, the frame in flight, the voice window of ALL the block's
// chunk steps, the block's slice of the output accumulator), the four programs, epilogue (state and frame out, emit:
// MyBuffer.cpp:113-133).
// This file is expanded TWICE by vp_pitch_ws.inc: as pitch_ws_body (one block per launch: the text of round 5's kernel, untouched --
// a template parameter with `if constexpr` branches in its place cost the single-block kernel 0.7 %, measured on one box) and, with
// WS_MB defined, as pitch_ws_body_mb (round 6, vp_k_pitch_ws_mb): mbp->nBlocks queued blocks in one launch.  There block 0 takes the
// prologue below, the last one the epilogue; in between a BOUNDARY (ws_mb_boundary) stands in for both: the finished block's samples
// leave (no state, no frame, no accumulator ring touched in HBM), the voice window is shifted by N samples inside LDS and topped up
// from the input slabs (ONE round of loads), the accumulator slice is shifted, the whole-ring gate is updated incrementally, the frame
// in flight is moved to the parity-0 buffers if it ended in the others.  Same arithmetic on the same data as block-by-block
// launches: same bits.
// A THIRD expansion, with WS_LEAN defined, is pitch_ws_body_l (vp_k_pitch_ws_l): see there.
#ifdef WS_MB
template <bool FAST, bool BIG>
__device__ __forceinline__ void pitch_ws_body_mb(const VpGeom &g_, const VpCall &c_, const VpDev &d_, const VpWsMb *mbp, const float *__restrict__ in,
                                                 float *__restrict__ out, double *smem)
{
    // mutable per-block copies of the arguments, laundered per block (ws_mb_launder) so that nothing derived from them is hoisted in
    // front of the block loop and carried across every program -- round 5's attempt at this loop died of 340 spilled registers
    VpGeom g = g_;
    VpCall c = c_;
    VpDev d = d_;
    const VpWsSched *scp = &mbp->sc[mbp->schedOf[0]];
    c.inCounter = mbp->inCtr[0]; c.outCounter = mbp->outCtr[0]; c.currCounter = mbp->currCtr[0]; c.nChunk0 = mbp->nChunk0[0];
    ws_mb_launder(g, c, d);
#define sc (*scp)
#elif defined(WS_LEAN)
// The LEAN expansion (vp_k_pitch_ws_l): the single-block FAST kernel for the one launch shape the host selects it for (vp_capi.hip
// pitch_ws_lean_ok) -- pitch corrector alone with both fusions, certified YIN, the plugin's geometry at 44.1 kHz, the `vec` prologue.
// What that shape fixes is written into private copies of the arguments as CONSTANTS, so every path it never takes (the one-sample
// prologue, ingest_gate_block, the unfused emit, the yinCert 0 / 2 entries, EXACT, the orders above 15) folds away and the chunk's
// divisions, trip counts and loop bounds are immediates.  Same routines, same order of every ordered sum: same bits.
__device__ __forceinline__ void pitch_ws_body_l(const VpGeom &g_, const VpCall &c_, const VpDev &d_, const VpWsSched &sc, const float *__restrict__ in,
                                                float *__restrict__ out, double *smem)
{
    constexpr bool FAST = true, BIG = false;
    VpGeom g = g_;
    g.F = WS_LEAN_F; g.C = WS_LEAN_C; g.H = WS_LEAN_F - WS_LEAN_C; g.cpf = 4; g.toKeep = WS_LEAN_F; g.eLen = 2 * WS_LEAN_F + 3 * WS_LEAN_C;
    g.orderPitch = WS_LEAN_ORDER; g.tauMax = WS_LEAN_TAUMAX;
    VpCall c = c_;
    c.fuseIngest = 1; c.fuseEmit = 1; c.vocOn = 0; c.pitchOn = 1; c.yinCert = 1; c.iirFast = 1; c.pStart = 0;
    VpDev d = d_;
    d.outAcc2 = nullptr;
#else
template <bool FAST, bool BIG>
__device__ __forceinline__ void pitch_ws_body(const VpGeom &g, const VpCall &c, const VpDev &d, const VpWsSched &sc, const float *__restrict__ in,
                                              float *__restrict__ out, double *smem)
{
#endif
    const int s = vp_stream(d), nt = blockDim.x, tid = vp_tid();
    const int nSteps = c.nSteps;
    VP_POISON(smem, c.ldsBytes);
    STAMP0(d);
#ifdef VP_STAMPS
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&WS_SLOT(d, 15, 7), (unsigned long long)wall_clock64());
#endif
    {   // the schedule sits in the kernel-argument segment: its cache lines are requested now, beside the prologue's loads, instead of
        // missing one after the other when the programs first index it
        const int *ws_ = (const int *)&sc;
        int acc_ = 0;
#pragma unroll
        for (int q = 0; q < (int)(sizeof(VpWsSched) / sizeof(int)); q += 16) acc_ += ws_[q];
        asm volatile("" :: "s"(acc_));
    }
    const bool fusedPro = c.fuseIngest && !c.vocOn;
    if (c.fuseIngest && !fusedPro) ingest_gate_block(g, c, d, in);
    lds_f64 *sm = (lds_f64 *)smem;
#ifdef WS_MB
    WsCarve cv = ws_carve(g, nSteps);
#else
    const WsCarve cv = ws_carve(g, nSteps);
#endif
    lds_ctl *ctl = (lds_ctl *)(sm + cv.ctl);
    lds_state *st = (lds_state *)(sm + cv.st), *stBG = st + 1;
    lds_f64 *xsAll = sm + cv.xs + ((g.toKeep - g.tauMax) & 1);
    lds_f64 *oE0 = sm + cv.fr, *yF0 = oE0 + g.F, *oA = sm + cv.oA;
    const float *vr = d.voiceRing + (size_t)s * g.inSize;
    const int pS0 = c.pStart;
    const int span = g.toKeep + g.F + (nSteps - 1) * g.C;

#ifdef WS_MB
    __shared__ double gateRed[17];                                            // ([16]: see ws_mb_boundary)
#else
    __shared__ double gateRed[16];
#endif
    // Everything the block needs from HBM is REQUESTED first -- every loop below only loads into registers, a fixed number of
    // (predicated) trips each, so the requests leave back to back -- and consumed afterwards: loop after loop of load -> convert ->
    // store paid one memory round trip per loop, eleven of them (6 us of prologue).
    constexpr int TR = 8;                              // trips of the ring-sized loops (whatever is beyond takes the plain loops at the end)
    const int mono = c.inMono;
    const float *xin = in + (size_t)s * (mono ? 1 : 3) * g.N;
    float gv[TR], xv[TR], wv0[4], wv1[4], wv2[4];
    double av[4], ov[2], yv = 0.0, hv = 0.0, a0v = 0.0;
    int sv_[2];
    d2 tv[2];
    const int idx0 = pS0 - g.toKeep;                                          // logical index of xsAll[0] (MyBuffer.cpp:152)
    const int p0 = ring_pos(c.currCounter, idx0, g.inSize);
    const int done0 = c.nChunk0 * g.C;
    // FOUR samples (two accumulator entries) per lane and request where the geometry allows -- every count and counter a multiple of four,
    // everything within one trip: the common case -- : what bounds this phase is the number of load INSTRUCTIONS the CU's memory
    // pipeline takes per microsecond (41 per thread in the one-sample form, 3.4 us until the last one has left)
    typedef float f4v __attribute__((ext_vector_type(4)));
    typedef double d2v __attribute__((ext_vector_type(2)));
#ifdef WS_LEAN
    constexpr bool vec = true;                                                // (the host launches this build only where vp_ws_vec_ok holds)
#else
    // (vp_common.h vp_ws_vec_ok restates this for the host, which asks it before it picks the lean build; tests/test_ws_lean_cpu.py holds
    // the two together.  The text stays here: routed through the helper, the generic builds' machine code moved)
    const bool vec = ((g.N | g.inSize | c.inCounter | p0 | (idx0 - g.latency) | span) & 3) == 0 && ((c.outCounter | g.outSize | (g.N + g.C)) & 1) == 0 &&
                     g.inSize <= 4 * nt && span <= 4 * nt && g.N + g.C <= 2 * nt && (((size_t)xin | (size_t)vr) & 15) == 0;
#endif
    f4v gq = {0.f, 0.f, 0.f, 0.f}, xq = {0.f, 0.f, 0.f, 0.f}, w0q = {0.f, 0.f, 0.f, 0.f}, w1q = {0.f, 0.f, 0.f, 0.f}, w2q = {0.f, 0.f, 0.f, 0.f};
    d2v aq = {0.0, 0.0};
    if (vec) {
        if (fusedPro) {
            const int p = 4 * tid;
            if (p < g.inSize) {
                int k = p - c.inCounter;
                k += (k < 0) ? g.inSize : 0;                                  // positions p .. p + 3 hold samples k .. k + 3 of the block, if k < N
                gq = (k < g.N) ? *(const f4v *)(xin + k) : *(const f4v *)(vr + p);
            }
            if (p < g.N) {
                w0q = *(const f4v *)(xin + p);
                if (mono == 0) { w1q = *(const f4v *)(xin + g.N + p); w2q = *(const f4v *)(xin + 2 * g.N + p); }
            }
        }
        const int j = 4 * tid;
        if (j < span) {
            int pp = p0 + j;
            pp -= (pp >= g.inSize) ? g.inSize : 0;
            const int k = idx0 + j - g.latency;
            xq = (fusedPro && k >= 0 && k < g.N) ? *(const f4v *)(xin + k) : *(const f4v *)(vr + pp);
        }
        const int q = 2 * tid;
        if (q < g.N + g.C) {
            int pos = c.outCounter + q;
            pos -= (pos >= g.outSize) ? g.outSize : 0;
            aq = *(const d2v *)(d.outAcc + (size_t)s * g.outSize + pos);
        }
    } else {
    if (fusedPro) {
        // the gate's sum over the ring AS IT WILL STAND: the block's own positions from the slab
#pragma unroll
        for (int u = 0; u < TR; u++) {
            const int p = tid + u * nt;
            int k = p - c.inCounter;
            k += (k < 0) ? g.inSize : 0;                                      // position p holds sample k of the block, if k < N
            gv[u] = (p < g.inSize) ? ((k < g.N) ? xin[k] : vr[p]) : 0.0f;
        }
        // MyBuffer::fillInputBuffers (MyBuffer.cpp:74-105): the block's samples for the ring write
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = tid + u * nt;
            wv0[u] = (i < g.N) ? xin[i] : 0.0f;
            wv1[u] = (i < g.N && mono == 0) ? xin[g.N + i] : 0.0f;
            wv2[u] = (i < g.N && mono == 0) ? xin[2 * g.N + i] : 0.0f;
        }
    }
    // the voice window of the block's steps: ring positions the block is about to overwrite come from the slab
#pragma unroll
    for (int u = 0; u < TR; u++) {
        const int j = tid + u * nt;
        int pp = p0 + j;
        pp -= (pp >= g.inSize) ? g.inSize : 0;                                // span < inSize: one wrap at most
        const int k = idx0 + j - g.latency;                                   // the block sits at logical [latency, latency + N)
        xv[u] = (j < span) ? ((fusedPro && k >= 0 && k < g.N) ? xin[k] : vr[pp]) : 0.0f;
    }
    {
        const double *acc = d.outAcc + (size_t)s * g.outSize;
#pragma unroll
        // (the ring positions by a conditional subtraction: a modulo by a run-time value is forty vector instructions, and the loads
        // cannot leave before their addresses exist -- outCounter < outSize and q < N + C <= outSize)
        for (int u = 0; u < 4; u++) {
            const int q = tid + u * nt;
            int pos = c.outCounter + q;
            pos -= (pos >= g.outSize) ? g.outSize : 0;
            av[u] = (q < g.N + g.C) ? acc[pos] : 0.0;
        }
    }
    }
    {
        const int *src = (const int *)(d.pitch + s);
#pragma unroll
        for (int u = 0; u < 2; u++) { const int i = tid + u * nt; sv_[u] = (i < (int)(sizeof(VpPitchState) / sizeof(int))) ? src[i] : 0; }
    }
    if (c.nChunk0 != 0) {
        // a frame may be in flight (parity 0 of this launch): the not yet filtered part of outEFrame, the recursion's history, the
        // impulse response of its 1/A(z), its coefficients (the residual is the producers' to fetch)
        const double *go = d.outEFrame + (size_t)s * g.F, *gy = d.yFrame + (size_t)s * g.F;
#pragma unroll
        for (int u = 0; u < 2; u++) { const int i = done0 + tid + u * nt; ov[u] = (i < g.F) ? go[i] : 0.0; }
        { const int i = max(0, done0 - g.orderPitch) + tid; if (i < done0) yv = gy[i]; }
        if (tid < (BIG ? 2 * WAVE : WAVE)) hv = d.hImp[(size_t)s * 2 * WAVE + tid];
        if (tid < WS_AF(g) && tid <= g.orderPitch) a0v = d.pitch[s].a[tid];
    }
    {   // the wavefront FFT's twiddle tables (13 KB, L2-resident), once per launch
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int i = tid + u * nt;
            tv[u] = i < 64 ? ((const d2 *)d.fftTw1)[(i >> 3) * 64 + (i & 7)] : i < 64 + 512 ? ((const d2 *)d.fftTw2)[i - 64]
                                                                             : i < 64 + 512 + 256 ? ((const d2 *)d.fftTws)[i - 64 - 512] : d2{0.0, 0.0};
        }
    }
    // ---- consume
    WS_EV0(d, 1, 0);                                   // (diagnostic: wavefront 0's prologue, in wavefront 1's spare slots: requests issued ...)
    if (vec) {
        if (fusedPro) {
            float *vrw = d.voiceRing + (size_t)s * g.inSize;
            double sv = 0.0;
            { const double a0 = (double)gq.x, a1 = (double)gq.y, a2 = (double)gq.z, a3 = (double)gq.w; sv += a0 * a0; sv += a1 * a1; sv += a2 * a2; sv += a3 * a3; }
            sv = wave_sum(sv);
            if ((tid & 63) == 0) gateRed[tid >> 6] = sv;
            const int i = 4 * tid;
            if (i < g.N) {
                int p = c.inCounter + i;
                p -= (p >= g.inSize) ? g.inSize : 0;                          // (inCounter < inSize, i < N <= inSize; multiples of four: no wrap inside the four)
                *(f4v *)(vrw + p) = w0q;
                if (mono != 2) {
                    float *sr0 = d.synthRing + (size_t)s * 2 * g.inSize;
                    *(f4v *)(sr0 + p) = w1q;
                    *(f4v *)(sr0 + g.inSize + p) = w2q;
                }
            }
        }
        const int j = 4 * tid;
        if (j < span) { xsAll[j] = (double)xq.x; xsAll[j + 1] = (double)xq.y; xsAll[j + 2] = (double)xq.z; xsAll[j + 3] = (double)xq.w; }
        const int q = 2 * tid;
        if (q < g.N + g.C) { oA[q] = aq.x; oA[q + 1] = aq.y; }
    } else {
    if (fusedPro) {
        float *vrw = d.voiceRing + (size_t)s * g.inSize;
        double sv = 0.0;
#pragma unroll
        for (int u = 0; u < TR; u++) { const double a = (double)gv[u]; sv += a * a; }
        for (int p = tid + TR * nt; p < g.inSize; p += nt) {                  // (rings beyond TR trips)
            int k = p - c.inCounter;
            k += (k < 0) ? g.inSize : 0;
            const double a = (double)((k < g.N) ? xin[k] : vr[p]);
            sv += a * a;
        }
        sv = wave_sum(sv);
        if ((tid & 63) == 0) gateRed[tid >> 6] = sv;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = tid + u * nt;
            if (i < g.N) {
                int p = c.inCounter + i;
                p -= (p >= g.inSize) ? g.inSize : 0;                          // (inCounter < inSize, i < N <= inSize)
                vrw[p] = wv0[u];
                if (mono != 2) {
                    float *sr0 = d.synthRing + (size_t)s * 2 * g.inSize;
                    sr0[p] = wv1[u];
                    sr0[g.inSize + p] = wv2[u];
                }
            }
        }
        for (int i = tid + 4 * nt; i < g.N; i += nt) {                        // (blocks beyond four trips)
            const int p = (c.inCounter + i) % g.inSize;
            vrw[p] = xin[i];
            if (mono != 2) {
                float *sr0 = d.synthRing + (size_t)s * 2 * g.inSize;
                sr0[p] = mono ? 0.0f : xin[g.N + i];
                sr0[g.inSize + p] = mono ? 0.0f : xin[2 * g.N + i];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < TR; u++) { const int j = tid + u * nt; if (j < span) xsAll[j] = (double)xv[u]; }
    for (int j = tid + TR * nt; j < span; j += nt) {
        int pp = p0 + j;
        pp -= (pp >= g.inSize) ? g.inSize : 0;
        const int k = idx0 + j - g.latency;
        xsAll[j] = (double)((fusedPro && k >= 0 && k < g.N) ? xin[k] : vr[pp]);
    }
    {
        const double *acc = d.outAcc + (size_t)s * g.outSize;
#pragma unroll
        for (int u = 0; u < 4; u++) { const int q = tid + u * nt; if (q < g.N + g.C) oA[q] = av[u]; }
        for (int q = tid + 4 * nt; q < g.N + g.C; q += nt) oA[q] = acc[(c.outCounter + q) % g.outSize];
    }
    }
    {   // state in: the producers' copy and the background's
        lds_i32 *dst = (lds_i32 *)st, *dst2 = (lds_i32 *)stBG;
#pragma unroll
        for (int u = 0; u < 2; u++) { const int i = tid + u * nt; if (i < (int)(sizeof(VpPitchState) / sizeof(int))) { dst[i] = sv_[u]; dst2[i] = sv_[u]; } }
    }
    if (c.nChunk0 != 0) {
        const double *go = d.outEFrame + (size_t)s * g.F;
#pragma unroll
        for (int u = 0; u < 2; u++) { const int i = done0 + tid + u * nt; if (i < g.F) oE0[i] = ov[u]; }
        for (int i = done0 + tid + 2 * nt; i < g.F; i += nt) oE0[i] = go[i];
        { const int i = max(0, done0 - g.orderPitch) + tid; if (i < done0) yF0[i] = yv; }
        lds_f64 *hp0 = sm + cv.hp;
        if (tid < WAVE) hp0[tid] = 0.0;
        if (tid < (BIG ? 2 * WAVE : WAVE)) hp0[WAVE + tid] = hv;
        if (tid < WS_AF(g)) (sm + cv.aF)[tid] = a0v;
    }
    {
        lds_d2 *tw = (lds_d2 *)(sm + cv.tw);
#pragma unroll
        for (int u = 0; u < 2; u++) { const int i = tid + u * nt; if (i < VP_FFT_TW_D2) tw[i] = tv[u]; }
    }
    // the control block: counters from zero (the schedule itself is a kernel argument)
    for (int i = tid; i < (int)(sizeof(WsCtl) / sizeof(int)); i += nt) ((lds_i32 *)ctl)[i] = 0;
#ifdef WS_LEAN
    if (tid == 0) ws_lean_tmo[0] = 0;                                           // (a wait that runs out leaves its mark here: raised once, below)
#endif
    if (tid >= nt / WAVE && tid < 16) gateRed[tid] = 0.0;                     // (the gate's sum takes all sixteen slots)
    WS_EV0(d, 1, 1);                                   // ... consumed ...
    __syncthreads();
    WS_EV0(d, 1, 2);                                   // ... barrier passed
    int gateOpen;
#ifdef WS_MB
    double gateT = 0.0;                                                       // the ring's sum of squares, carried from block to block
#endif
    if (fusedPro) {
        // the gate's verdict (see ingest_gate_block): every thread sums the eight wave totals in the same order; inside the
        // rounding band of the threshold thread 0 redoes the reference's sequential sum over the (now complete) ring
        // (all sixteen slots, the unused ones zero -- adding +0.0 changes nothing --: four wide LDS reads in one batch instead of a
        // loop whose tail pays an LDS round trip per wavefront; this runs on every wavefront right behind the barrier)
        double T = 0.0;
#pragma unroll
        for (int w = 0; w < 16; w++) T += gateRed[w];
#ifdef WS_MB
        gateT = T;
        if (tid == 0) gateRed[16] = T;                                        // the largest T since the last exact sum (ws_mb_boundary)
#endif
        const double band = T * vp_f64_here(2 * g.inSize + 64) * 1.1102230246251565e-16 * 1.5;
        if (T - g.gateThrSum > band) gateOpen = 1;
        else if (g.gateThrSum - T > band) gateOpen = 0;
        else {
            if (tid == 0) {
                double seq = 0.0;                                             // AudioBuffer::getRMSLevel order
                for (int i = 0; i < g.inSize; i++) { double a = (double)vr[i]; seq += a * a; }
                ctl->ishareP[0] = !(seq < g.gateThrSum);
            }
            __syncthreads();
            gateOpen = ctl->ishareP[0];
            __syncthreads();
        }
        if (tid == 0) d.gate[s * 2 + 0] = gateOpen;
    } else
        gateOpen = d.gate[s * 2 + 0];
    STAMP(d, 15);
    const double gainPitch = st->sp.gainPitch;
#ifndef WS_MB
    const int nInst = sc.nInst;
#endif
    const int wv = tid >> 6;
#ifdef WS_MB
    {
        // the accumulator ring's entries this call has taken into LDS: zero in HBM now (the call's last block leaves its overhang behind
        // the LAST block's position; block-by-block launches clear a block's own region at emit and rewrite the overhang every time)
        double *acc = d.outAcc + (size_t)s * g.outSize;
        for (int q = tid; q < g.N + g.C; q += nt) {
            int pos = c.outCounter + q;
            pos -= (pos >= g.outSize) ? g.outSize : 0;
            acc[pos] = 0.0;
        }
    }
    const float *inb = in;
    float *outb = out;
    const int nB = mbp->nBlocks;
    for (int blk = 0; ; blk++) {
#endif

    // ---- the four programs (no workgroup barrier in here) ----
    // wavefronts [0, nRec): recursion; [nRec, NW - 4): producers (the first of them owns the grain tables); the last four: background
    const int NW = nt / WAVE, nRec = FAST ? 1 : 2, nFG = FAST ? 2 : 2, nP = NW - WS_NBG - nFG;   // (FAST: wavefront 1 adds the recursion's outputs)
    if (wv >= NW - WS_NBG)
    {
        // (which of the four takes which rank: the lead on the SIMD it shares with the windowed-add wavefront -- mostly asleep -- and one
        // producer, rather than with two producers: +0.8 %, measured on one box against three other placements)
        const int x = wv - (NW - WS_NBG);
        ws_background<FAST, BIG, WS_IS_LEAN>(g, c, d, sc, sm, cv, ctl, FAST ? (0x1230 >> (4 * x)) & 15 : x, gateOpen);   // (EXACT: wavefront 1 is a recursion wavefront; the lead stays last)
    }
    else if (wv < nRec)
        ws_recursion<FAST, BIG, WS_IS_LEAN>(g, c, d, sc, sm, cv, ctl, wv, nRec, gainPitch);
    else if (FAST && wv == 1)
        ws_filler<WS_IS_LEAN>(g, c, d, sc, sm, cv, ctl, gainPitch);
    else
#ifdef WS_MB
        ws_producer<FAST, WS_IS_LEAN>(g, c, d, sc, sm, cv, ctl, wv - nFG, nP, gateOpen, blk == 0, blk == nB - 1);
    if (blk != nB - 1) ws_lds_barrier(); else
    __syncthreads();
    if (blk == nB - 1) break;
    ws_mb_boundary(g, c, d, mbp, blk, scp, sm, cv, ctl, st, stBG, xsAll, oE0, yF0, oA, gateRed, inb, outb, span, gateT, gateOpen);
    }
#define out outb
#else
        ws_producer<FAST, WS_IS_LEAN>(g, c, d, sc, sm, cv, ctl, wv - nFG, nP, gateOpen);
    __syncthreads();
#endif
    STAMP(d, 8);

    // ---- epilogue ----
#ifdef WS_MB
    const int nInst = sc.nInst;                                               // (the last block's schedule)
#endif
    {
        const int tid = vp_tid();
        {   // state out
            int *dst = (int *)(d.pitch + s);
            const lds_i32 *src = (const lds_i32 *)st;
            for (int i = tid; i < (int)(sizeof(VpPitchState) / sizeof(int)); i += nt) dst[i] = src[i];
        }
        // the frame in flight at the end of the block: the last instance's (every step leaves nChunk >= 1)
        const int pl = sc.instPar[nInst - 1];
        int nChunkEnd = c.nChunk0;
        for (int t = 0; t < nSteps; t++) { if (nChunkEnd == g.cpf - 1) nChunkEnd = 0; nChunkEnd += 1; }
        if (nChunkEnd != 0 && st->nAn != 0) {
            double *go = d.outEFrame + (size_t)s * g.F, *gy = d.yFrame + (size_t)s * g.F;
            const lds_f64 *oEl = pl ? oE0 + 3 * g.F + 2048 : oE0, *yFl = pl ? oE0 + 2 * g.F + 2048 : yF0;
            const int done = nChunkEnd * g.C;
            for (int i = done + tid; i < g.F; i += nt) go[i] = oEl[i];
            for (int i = max(0, done - g.orderPitch) + tid; i < done; i += nt) gy[i] = yFl[i];
            if (tid < (BIG ? 2 * WAVE : WAVE)) d.hImp[(size_t)s * 2 * WAVE + tid] = (sm + cv.hp + pl * WS_HP(g))[WAVE + tid];
        }
        STAMP(d, 11);
        // what the block's chunks left beyond its own N samples goes back to the accumulator ring (everything, when somebody
        // else emits); the block's own region is consumed -- and zeroed in HBM -- by emit_block
        double *acc = d.outAcc + (size_t)s * g.outSize;
        for (int q = (c.fuseEmit ? g.N : 0) + tid; q < g.N + g.C; q += nt) {
            int pos = c.outCounter + q;
            pos -= (pos >= g.outSize) ? g.outSize : 0;
            acc[pos] = oA[q];
        }
        if (c.fuseEmit) ws_emit_block(g, c, d, out, st, (const lds_f64 *)oA);
    }
#ifdef WS_LEAN
    // a bounded wait of this launch ran out (ws_wait_ge<true>): the fault word is raised here, once, still inside the launch -- the
    // host sees what it sees from the other builds (VP_ERR_TIMEOUT, a poisoned handle)
    if (tid == 0 && ws_lean_tmo[0] != 0) vp_timeout(vp_tmo(d, 61));
#endif
#ifdef VP_STAMPS
    if (blockIdx.x == 0 && threadIdx.x == 0) { atomicAdd(&WS_SLOT(d, 0, 7), 1ULL); atomicAdd(&WS_SLOT(d, 0, 5), (unsigned long long)wall_clock64()); }   // launches of this type; kernel end
#endif
#ifdef WS_MB
#undef out
#undef sc
#endif
}

