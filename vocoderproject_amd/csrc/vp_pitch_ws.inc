// vp_pitch_ws.inc -- part of vp_kernels.hip (included there, behind vp_pitch.inc whose device routines it calls).
//
// K2w: the pitch corrector (PitchProcess::process, PitchProcess.cpp:166-271) as a WAVE-SPECIALISED kernel (round 5).
//
// vp_k_pitch* (vp_pitch.inc) walks a block's chunk steps as barrier-separated phases of the whole workgroup: one dependent chain
// per stream, in whose serial stretches (marks, running sum, recursion) five to seven of their eight wavefronts wait.  But the
// reference's own data flow is much looser than its program order:
//   * everything processChunkStart derives from the INPUT (yin() :350-448, the frame's LPC :230-233, LPC.cpp:44-148) can be
//     computed as soon as the block is in the ring -- every frame that starts inside a block reads samples below
//     startSample + F <= latency + N (:221,233);
//   * the marks (:455-658) additionally need the previous frame's marks -- a short integer chain from Start to Start -- but
//     nothing the old frame's Cont chunks (:253-271) produce;
//   * a frame's chunks (residual -> PSOLA -> recursion -> windowed add) form a chain of their own per frame; two consecutive
//     frames share nothing but the order of their additions into the output.
// So the TWELVE wavefronts of the workgroup run FOUR programs side by side and meet through counters in LDS (no workgroup barrier
// between the prologue and the epilogue):
//   BACKGROUND (wavefronts 8..11): for every frame that starts inside the block, in order: certified YIN (cross-correlations by FFT,
//       one forward transform per wavefront), prefix sums, LPC autocorrelation -> Levinson-Durbin -> impulse response, then on the
//       lead wavefront the pick, pitchMarks and placeStMarks on a PRIVATE copy of the tracker state, which is then published.
//       All of it beside the old frame's chunks.
//   PRODUCERS (wavefronts 2..7): the block's SEGMENTS (the chunks of one frame that this block's steps run) in order: residual
//       (filterFIR :280-302), one grain table per segment (wavefront 2), one gather pass of psola() (:665-741) in trips of 64 output
//       samples that whichever wavefront is free takes; a chunk is released to the recursion by whoever finishes its last trip.
//       At a Start the table is built from the published copy while another wavefront adopts it for the group.
//   RECURSION (wavefront 0; EXACT: wavefronts 0 and 1, alternate frames): filterIIR (:307-322) of every instance as soon as its
//       stretch of outEFrame is complete.
//   WINDOWED ADD (FAST: wavefront 1; EXACT: the recursion wavefronts themselves): fillOutputBuffer (:328-342), additions to the
//       output in the reference's order (a turn counter).
// The frame buffers the two kinds of consumers share are double-buffered by FRAME PARITY (outEFrame, yFrame, the coefficients
// and the impulse response); eFrame, the quotient / Hann tables and the grain table belong to the producers alone and follow
// the instance order, so one copy serves.  The FFT's exchange buffers live in the NEXT frame's (still unused) outEFrame/yFrame.
//
// Same device routines as vp_k_pitch_fast_c / vp_k_pitch_c, same arithmetic, same order of every ordered sum: the output is
// bit-identical to theirs (EXACT: to the oracle's).  Geometry: the common case with F = 1024 (vp_capi.hip pitch_ws_ok);
// everything else keeps the phase kernels.
//
// Every wait is bounded, and a wait that runs out is an ERROR (vp_timeout: the handle's fault word in pinned host memory; the host
// fails the call with VP_ERR_TIMEOUT and poisons the handle) -- never a hung GPU, never silently wrong audio.

// Diagnostic build (-DVP_STAMPS): workgroup 0's wavefronts accumulate, per block type (nChunk at entry) and wavefront, event times
// since kernel entry (WS_EV) and durations (WS_TB / WS_TA) into dbg[64 + S + type * 128 + wave * 8 + slot] (tools/ws_stamps.py, through
// vp_debug_read_ws_stamps).  Slot 7 of wavefront 0 counts the launches.
#ifdef VP_STAMPS
// (fire-and-forget atomics of ABSOLUTE clock values, the launches' entry times summed in slot (15, 7) and subtracted by the tool: a
// read-modify-write or a load of the entry time would stall the stamping wavefront for a memory round trip per stamp)
#define WS_SLOT(D, W, E) (D).dbg[64 + g.S + (c.nChunk0 & 3) * 128 + (W) * 8 + (E)]
#define WS_EV(D, W, E) do { if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) atomicAdd(&WS_SLOT(D, W, E), (unsigned long long)wall_clock64()); } while (0)
#define WS_EV0(D, W, E) do { if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&WS_SLOT(D, W, E), (unsigned long long)wall_clock64()); } while (0)
#define WS_TB() unsigned long long ws_tb_ = wall_clock64()
#define WS_TA(D, W, E) do { if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) { const unsigned long long t_ = wall_clock64(); atomicAdd(&WS_SLOT(D, W, E), t_ - ws_tb_); ws_tb_ = t_; } } while (0)
#define WS_TR() do { ws_tb_ = wall_clock64(); } while (0)
#define WS_FINE(D, K) do { if (i == 0) WS_EV(D, 12 + (K) / 8, (K) % 8); } while (0)
#define WS_FINEP(D, K) do { if (si == 0 && rank < 2) WS_EV(D, 13 + rank, K); } while (0)   // (producers 0 and 1, the first Start's segment; the recursion's instances: wavefront 15)
#define WS_FINER(D, J) do { if ((J) < 7) WS_EV(D, 15, J); } while (0)
#define WS_STAT(D, K, V) do { if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) atomicAdd(&(D).dbg[64 + g.S + (K)], (unsigned long long)(V)); } while (0)   // (ad-hoc counters in block type 0's slots: the bench's cohort never has it)
#define WS_CLK() wall_clock64()      // (the lead's first start in detail: the slots of wavefronts that do not exist)
#else
#define WS_EV(D, W, E) do { } while (0)
#define WS_EV0(D, W, E) do { } while (0)
#define WS_TB() do { } while (0)
#define WS_TA(D, W, E) do { } while (0)
#define WS_TR() do { } while (0)
#define WS_FINE(D, K) do { } while (0)
#define WS_FINEP(D, K) do { } while (0)
#define WS_FINER(D, J) do { } while (0)
#define WS_STAT(D, K, V) do { } while (0)
#define WS_CLK() 0ULL
#endif

// The control block is addressed as LDS (ds_read / ds_add): a poll through a generic pointer is a flat access, several times the latency.
typedef __attribute__((address_space(3))) WsCtl lds_ctl;
// (a wait that runs out is an ERROR: vp_timeout raises the handle's fault word and the host fails the call -- what the wait was for is
// not there, so the launch's output is void; d.spinLimit polls ~ a second)
// LEAN (vp_k_pitch_ws_l; every program below carries the switch down to its waits): a wait that runs out only leaves a mark in LDS,
// and the launch raises the fault word once, at its end (pitch_ws_body_l) -- the fifty wait sites of the four programs then carry one
// LDS store each instead of an atomic, a system-scope store and their lane masks.
// (sixteen bytes, aligned: the kernel's dynamic LDS starts behind its static LDS, and the FFT's exchange buffers and twiddles in it are
// read and written sixteen bytes at a time -- with a static part of 8 mod 16 bytes (a 4-byte mark) every one of those accesses was
// misaligned and the launch 9 us longer, measured: profiles/ws_lean_ab.txt)
__shared__ __attribute__((aligned(16))) int ws_lean_tmo[4];
template <bool LEAN = false>
__device__ __forceinline__ void ws_wait_ge(lds_i32 *flag, int target, const VpDev &d)
{
    int spin = 0;
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < target) {
        if (++spin >= d.spinLimit) {
            if constexpr (LEAN) ws_lean_tmo[0] = 1;
            else if ((vp_tid() & 63) == 0) vp_timeout(vp_tmo(d, 61));
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}
__device__ __forceinline__ void ws_signal(lds_i32 *flag, int value)
{
    __threadfence_block();
    if ((vp_tid() & 63) == 0) __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// barrier of a GROUP of n wavefronts: a monotone counter, `gen` the caller's count of barriers passed (uniform in the group)
template <bool LEAN = false>
__device__ __forceinline__ void ws_group_barrier(lds_i32 *ctr, int n, int &gen, const VpDev &d)
{
    gen += 1;
    __threadfence_block();
    if ((vp_tid() & 63) == 0) __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    ws_wait_ge<LEAN>(ctr, n * gen, d);
}

// exclusive prefix sums P[j] of w_j^2, j <= nb, by one wavefront (what wave 5 does in pitch_chunk_start_pre; same additions in the same
// order) -- with the lane's entries requested at once (nb <= 24 * 64): the plain loop is one LDS round trip per entry and pass,
// 4.5 us on the background's critical path.
__device__ __forceinline__ void ws_prefix_sums(const lds_f64 *w, lds_f64 *P, int nb)
{
    asm volatile("" : "+s"(nb));                                              // (its two dozen uniform masks are made here, not at the top of the kernel)
    const int lane = vp_tid() & 63, per = (nb + WAVE - 1) / WAVE, j0 = lane * per;
    double v[24];
#pragma unroll
    for (int u = 0; u < 24; u++) { const int j = j0 + u; v[u] = (u < per && j < nb) ? w[min(j, nb - 1)] : 0.0; }
    double loc = 0.0;
#pragma unroll
    for (int u = 0; u < 24; u++) { const int j = j0 + u; if (u < per && j < nb) loc += v[u] * v[u]; }
    double inc = loc;
    for (int off = 1; off < WAVE; off <<= 1) { const double o = __shfl_up(inc, off, WAVE); if (lane >= off) inc += o; }
    double run = inc - loc;
#pragma unroll
    for (int u = 0; u < 24; u++) { const int j = j0 + u; if (u < per && j <= nb) { P[j] = run; if (j < nb) run += v[u] * v[u]; } }
}

// yin() from the normalisation on (PitchProcess.cpp:395-403, 431-440) in the reference's arithmetic, by ONE wavefront: yin_pick with
// cert = 0, without its workgroup barriers.  dY holds the reference's sums, cum their running sum.
__device__ __forceinline__ void ws_yin_pick_wave(const VpGeom &g, const VpDev &d, const PitchLds &L, lds_state *st)
{
    const int lane = vp_tid() & 63;
    for (int k = 1 + lane; k < g.tauMax; k += WAVE) {
        const double cm = L.cum[k], q = (double)k / cm;
        L.dY[k] = L.dY[k] * q;
    }
    wave_sync();
    int tau = INT_MAX;
    for (int k0 = g.tau0; k0 < g.tauMax; k0 += WAVE) {                        // first tau with d < tol (:431-433)
        const int k = k0 + lane;
        const unsigned long long m = __ballot(k < g.tauMax && L.dY[min(k, g.tauMax - 1)] < g.yinTol);
        if (m) { tau = k0 + (int)__builtin_ctzll(m); break; }
    }
    if (tau < g.tauMax) {
        while (true) {                                                       // :435-440 (uniform: every lane walks)
            const double a = L.dY[tau + 1], b = L.dY[tau];
            if (!(a < b)) break;
            tau += 1;
            if (tau + 1 >= g.tauMax) break;
        }
        if (lane == 0) {
            if (tau >= g.tauMax) atomicAdd(&d.ub[3], 1ULL);
            st->pitch = g.fs / tau;
            st->period = tau;
        }
    }
}


// ------------------------------------------------------------------------------------------------
// psola() (PitchProcess.cpp:665-741) for a SEGMENT -- the chunks kFirst..kLast of one frame, which this block's steps
// tFirst, tFirst + 1, ... run -- in one table and one gather pass.  The reference walks the chunks one after the other; what a
// chunk k contributes is, per synthesis mark that falls due in it (:685, stMark - T < (k + 1) C), one grain, added into outEFrame
// from position k C on (earlier positions have been filtered: dead, see psola_pass2) and read from an eFrame whose entries from
// toKeep + F + k C on are still zero (:216, :258-259).  The marks ascend, so the chunk a pending mark falls due in is
// max(kFirst, floor((stMark - T) / C)), non-decreasing along the marks: one lane per mark builds all the segment's grains at
// once, each with its own chunk's closest-analysis-mark test (:788-831 depends on nChunk and startSample), first position and
// eFrame limit; the gather then adds, per output sample, the grains that cover it in mark order -- the order in which the
// reference's interp() calls reach that sample (chunk by chunk, mark by mark).
struct SegTab {
    lds_f64 *x0, *xN;                                      // [VP_MARKS]
    lds_i32 *stMark, *srcBase, *flags, *startIdx, *stopIdx, *eLim;   // [VP_MARKS]
};
__device__ __forceinline__ SegTab ws_seg_tab(lds_f64 *base)
{
    SegTab G;
    G.x0 = base; G.xN = base + VP_MARKS;
    G.stMark = (lds_i32 *)(base + 2 * VP_MARKS); G.srcBase = G.stMark + VP_MARKS; G.flags = G.srcBase + VP_MARKS;
    G.startIdx = G.flags + VP_MARKS; G.stopIdx = G.startIdx + VP_MARKS; G.eLim = G.stopIdx + VP_MARKS;
    return G;
}
// by ONE wavefront (lane = pending mark).  Leaves the number of grains in *ngOut and advances st->stMarkIdx.
// (st: the frame's tracker state, read only -- at a Start the background's published copy, which the group adopts meanwhile --;
// stIdx: the group's own copy, whose chunk progress stMarkIdx this advances)
// park: the segment's producers park the recursion's first pass behind their trips (VpWsSched::segPark) -- the pass then covers the
// segment's chunks whole, from the first one's first sample, in trips aligned to the recursion's 64-sample blocks (chunks are
// multiples of 64 samples here): every block of every instance is some trip's, so no instance is ever parked in part.  Lanes and
// trips that no grain covers write back what they read.
__device__ __forceinline__ void ws_psola_table_seg(const VpGeom &g, const VpDev &d, const lds_state *st, lds_state *stIdx, const SegTab &G, int kFirst, int kLast,
                                                   int pSFirst, lds_ctl *ctl, int sg, bool park)
{
    const int lane = vp_tid() & 63;
    const int T = (st->pitch > 1) ? st->period : st->prevVoicedPeriod;
    const int nG = 2 * T + 1;
    const int nSt = st->nSt;
    const int smi0 = stIdx->stMarkIdx;
    const int smi = smi0 + lane;
    const bool have = smi < nSt;
    const int stMark = have ? st->stMarks[smi] : 0;
    // the chunk the mark falls due in: the first k >= kFirst with stMark - T < (k + 1) C
    const int v = stMark - T;
    const int kd = max(kFirst, v >= 0 ? v / g.C : 0);
    const bool due = have && kd <= kLast;
    const unsigned long long notDue = ~__ballot(due);
    const int ng = notDue ? (int)__builtin_ctzll(notDue) : 64;              // length of the due prefix
    if (lane < ng) {
        const int pS = pSFirst + (kd - kFirst) * g.C;                       // startSample of the step that runs chunk kd
        bool q2 = false;
        int clIdx = closest_an_mark_idx(g, st, stMark, T, kd, pS, q2);
        if (q2) atomicAdd(&d.ub[0], 1ULL);
        int clAnMark;
        if (clIdx >= 0)
            clAnMark = st->anMarks[clIdx];
        else {                                                               // Q3
            int j = st->nPrevAn - clIdx;
            atomicAdd(&d.ub[1], 1ULL);
            clAnMark = (j >= 0 && j < VP_MARKS) ? st->prevAnMarks[j] : 0;
        }
        const double dSt = (double)stMark;
        const double beta = st->beta;
        const double x0 = dSt + (double)(0 - T) / beta;                     // xInterp[0]
        const double xN = dSt + (double)(nG - 1 - T) / beta;                // xInterp.back()
        G.x0[lane] = x0; G.xN[lane] = xN;
        G.stMark[lane] = stMark;
        G.srcBase[lane] = g.toKeep + clAnMark - T;
        G.flags[lane] = (smi == 0 ? 1 : 0) | (smi == nSt - 1 ? 2 : 0);
        G.startIdx[lane] = max(max((int)floor(x0), 0), kd * g.C);
        G.stopIdx[lane] = min((int)ceil(xN), g.F);
        G.eLim[lane] = min(g.eLen, g.toKeep + g.F + kd * g.C);
    }
    // the gather pass's extent: marks ascend, the first grain starts first; trips of 64 samples from there to the last grain's end
    int lo = 0, hi = 0;
    if (lane < ng) { lo = G.startIdx[lane]; hi = G.stopIdx[lane]; }
    lo = __builtin_amdgcn_readfirstlane(lo);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hi = max(hi, __shfl_xor(hi, off, WAVE));
    if (park) { lo = kFirst * g.C; hi = max(hi, (kLast + 1) * g.C); }
    if (lane == 0) {
        stIdx->stMarkIdx = smi0 + ng;
        ctl->gNg[sg] = ng; ctl->gLo[sg] = lo; ctl->gHi[sg] = hi;
        ctl->gNT[sg] = ((ng > 0 || park) && hi > lo) ? (hi - lo + WAVE - 1) / WAVE : 0;
    }
}
// the gather: 64 consecutive output samples per trip.  Lane q holds grain q's entry in registers; the grains that touch a trip's
// samples are found by a ballot and their entries reach the lanes through readlane -- no LDS traffic for the (wave-uniform)
// entries, no search per sample.
// The trips are TAKEN, in ascending order, by whichever wavefront comes for one (gNext): the wavefront that owns the serial grain
// tables arrives late and takes few.  A trip belongs to the instance whose chunk its first sample lies in (clamped to the segment's
// chunks): an instance's stretch of outEFrame is complete once its own and all earlier trips are done -- later trips only write
// beyond it.  Whoever finishes an instance's last trip releases it to the recursion, in instance order (psDone).
// (Background wavefronts that had finished their starts took trips too, in one experiment: no gain beside the lead's SIMD-mates and a
// loss -- 4 % -- when the one that shares the recursion's SIMD joined in.  What bounds the pass is one trip's latency, not hands.)
// hpPark (a parked segment, else null): the frame's padded impulse response.  A trip's 64 samples are FINAL when the trip stores
// them -- every grain that covers a sample is added inside the trip that owns it, earlier segments' grains are in already, later
// segments' grains start at or beyond their own chunks -- so the trip's owner runs the recursion's first pass on that block right
// behind the store (iir_block_park into yFrame, which nobody reads there before the instance's recursion) -- for the blocks inside the
// segment's own chunks: what a grain spills beyond the last chunk is not final yet.  The taps are requested per trip: 96 registers of
// them do not fit beside the gather's state.  Parked instances are released with instMode 3.
template <bool LEAN = false>
__device__ __forceinline__ void ws_psola_gather_seg(const VpGeom &g, const VpDev &d, const PitchLds &L, const SegTab &G, lds_ctl *ctl, int sg, int jA, int jB,
                                                    int kFirst, bool first, const lds_f64 *hpPark = nullptr, int nChunk0 = 0)
{
    const lds_state *st = L.st;
    const int lane = vp_tid() & 63;
    const int nT = ctl->gNT[sg], lo = ctl->gLo[sg], hi = ctl->gHi[sg], ng = ctl->gNg[sg];
    const lds_f64 *hw = L.htab;
    // (the frame's and the table's entries: read with the first trip in hand -- a wavefront that holds a trip keeps the segment open,
    // and only an open segment's tables are stable)
    bool have = false;
    int T = 0, nG = 1;
    double beta = 1.0, mx0 = 0.0, mxN = 0.0;
    int mst = 0, msrc = 0, mfl = 0, ma = 0, mb = 0, mlim = 0;
    // trips whose first sample lies below x
    auto below = [&](int x) -> int { return (x <= lo) ? 0 : min((x - lo + WAVE - 1) / WAVE, nT); };
    // trips of instance jA + r: those that start in [r == 0 ? -inf : (kFirst + r) C, r == last ? +inf : (kFirst + r + 1) C)
    auto count = [&](int r) -> int {
        const int a = (r == 0) ? 0 : below((kFirst + r) * g.C), b = (r == jB - jA) ? nT : below((kFirst + r + 1) * g.C);
        return b - a;
    };
    // the release of instance j (and of the instances without trips of their own right behind it), once everything before it is out
    auto release = [&](int j) {
        ws_wait_ge<LEAN>(&ctl->psDone, j, d);
        for (;;) {
            if (lane == 0) ctl->instMode[j] = hpPark ? 3 : 2;
            ws_signal(&ctl->psDone, j + 1);
            j++;
            if (j > jB || count(j - jA) != 0) break;
        }
    };
    if (first) {                                                             // (the table's owner, before its first trip: instances without trips at the head)
        if (count(0) == 0) release(jA);
    }
    for (;;) {
        int m = 0;
        if (lane == 0) m = __hip_atomic_fetch_add((lds_i32 *)&ctl->gNext[sg], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        m = __builtin_amdgcn_readfirstlane(m);
        if (m >= nT) break;
        const unsigned long long tTrip0 = WS_CLK();
        (void)tTrip0;
        if (!have) {
            have = true;
            T = (st->pitch > 1) ? st->period : st->prevVoicedPeriod;
            nG = 2 * T + 1;
            beta = st->beta;
            const int ql = max(min(lane, ng - 1), 0);
            mx0 = G.x0[ql]; mxN = G.xN[ql];
            mst = G.stMark[ql]; msrc = G.srcBase[ql]; mfl = G.flags[ql]; ma = G.startIdx[ql]; mb = G.stopIdx[ql]; mlim = G.eLim[ql];
        }
        const int b = lo + WAVE * m;
        const int i = b + lane;
        const bool in = i < hi;
        const double di = (double)i;
        double accv = in ? L.oE[i] : 0.0;
        unsigned long long mask = __ballot(lane < ng && ma < b + WAVE && mb > b);
        // one grain's contribution to this lane's sample (interp :842-870 through the lower bound on the strictly increasing
        // x[j] = stMark + (j - T) / beta, :853); `act`: the sample lies in the grain
        struct Entry { int sa, sb, stM, srcBase, fl, eLim; double x0, xN; };
        auto entry = [&](int q) -> Entry {
            Entry e;
            e.sa = __builtin_amdgcn_readlane(ma, q); e.sb = __builtin_amdgcn_readlane(mb, q);
            e.x0 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(mx0), q), __builtin_amdgcn_readlane(__double2loint(mx0), q));
            e.xN = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(mxN), q), __builtin_amdgcn_readlane(__double2loint(mxN), q));
            e.stM = __builtin_amdgcn_readlane(mst, q); e.srcBase = __builtin_amdgcn_readlane(msrc, q); e.fl = __builtin_amdgcn_readlane(mfl, q);
            e.eLim = __builtin_amdgcn_readlane(mlim, q);
            return e;
        };
        // the general form: the search corrected by as many steps as it takes (exactly psola_pass2's)
        auto slow = [&](const Entry &e, bool &act) -> double {
            act = in && i >= e.sa && i < e.sb && di >= e.x0 && di <= e.xN;   // :852
            if (!act) return 0.0;
            const double dSt = (double)e.stM;
            int j = (int)ceil((di - dSt) * beta) + T;
            j = max(0, min(j, nG - 1));
            const double q0 = L.qtab[j], qm = L.qtab[max(j - 1, 0)], qp = L.qtab[min(j + 1, nG - 1)];
            double xj = dSt + q0, xjm = 0.0;
            if (j < nG - 1 && xj < di) {
                xjm = xj; j++; xj = dSt + qp;
                while (j < nG - 1 && xj < di) { xjm = xj; j++; xj = dSt + L.qtab[j]; }
            } else if (j > 0) {
                xjm = dSt + qm;
                if (xjm >= di) {
                    j--; xj = xjm;
                    while (j > 0) {
                        xjm = dSt + L.qtab[j - 1];
                        if (xjm >= di) { j--; xj = xjm; } else break;
                    }
                }
            }
            auto ys = [&](int jj) -> double {
                const int src = e.srcBase + jj;
                const double ev = (src >= 0 && src < e.eLim) ? L.eF[src] : 0.0;
                const bool windowed = (e.fl & 1) ? (jj >= T) : ((e.fl & 2) ? (jj < T) : true);   // :696-731 (first wins)
                return windowed ? ev * hw[jj] : ev;
            };
            if (j > 0) {
                const double ya = ys(j - 1), yb = ys(j);
                return ya + (yb - ya) / (xj - xjm) * (di - xjm);             // :860
            }
            return ys(0);
        };
        // the same without a branch, for the two outcomes the estimate j0 = ceil((i - stMark) beta) + T almost always has -- it IS the
        // lower bound, or the bound is the next entry --: every load unconditional (clamped), every decision a select, so that TWO
        // grains' chains of dependent LDS round trips and divisions run interleaved.  `ok`: this lane's sample is one of the two cases
        // (or not in the grain at all); otherwise the pair is redone by the general form.
        auto fast = [&](const Entry &e, bool &act, bool &ok) -> double {
            act = in && i >= e.sa && i < e.sb && di >= e.x0 && di <= e.xN;
            const double dSt = (double)e.stM;
            int j0 = (int)ceil((di - dSt) * beta) + T;
            j0 = max(0, min(j0, nG - 1));
            const double q0 = L.qtab[j0], qm = L.qtab[max(j0 - 1, 0)], qp = L.qtab[min(j0 + 1, nG - 1)];
            const double xj0 = dSt + q0, xm0 = dSt + qm, xp0 = dSt + qp;
            const bool up = j0 < nG - 1 && xj0 < di;
            const bool upMore = up && (j0 + 1 < nG - 1) && xp0 < di;
            const bool down = !up && j0 > 0 && xm0 >= di;
            ok = !act || !(upMore || down);
            const int j = up ? j0 + 1 : j0;
            const double xj = up ? xp0 : xj0, xjm = up ? xj0 : xm0;
            const int ja = max(j - 1, 0);
            const int srcA = e.srcBase + ja, srcB = e.srcBase + j;
            const double ea = L.eF[max(0, min(srcA, e.eLim - 1))], eb = L.eF[max(0, min(srcB, e.eLim - 1))];
            const double ha = hw[ja], hb = hw[j];
            const double eva = (srcA >= 0 && srcA < e.eLim) ? ea : 0.0, evb = (srcB >= 0 && srcB < e.eLim) ? eb : 0.0;
            const bool wa = (e.fl & 1) ? (ja >= T) : ((e.fl & 2) ? (ja < T) : true), wb = (e.fl & 1) ? (j >= T) : ((e.fl & 2) ? (j < T) : true);
            const double ya = wa ? eva * ha : eva, yb = wb ? evb * hb : evb;
            const double itp = ya + (yb - ya) / (xj - xjm) * (di - xjm);     // :860
            return (j > 0) ? itp : yb;
        };
        while (mask) {
            const int q1 = (int)__builtin_ctzll(mask);
            mask &= mask - 1;
            const bool two = mask != 0;
            const int q2 = two ? (int)__builtin_ctzll(mask) : q1;
            mask &= mask - 1;                                                // (mask == 0 stays 0)
            const Entry e1 = entry(q1), e2 = entry(q2);
            bool a1, a2, ok1, ok2;
            double v1 = fast(e1, a1, ok1), v2 = fast(e2, a2, ok2);
            WS_STAT(d, 2, 1);
#ifdef WS_GATHER_TEST
            // (tools/ws_gather_selftest.sh: the general form is all but unreachable with real signals -- 0 of 2953 pairs in the bench's
            // cohort --, so two side builds declare the branch-free form unfit for every pair (1) / for one lane of every other trip (2)
            // and run the parity suite on them)
            if (WS_GATHER_TEST == 1) ok1 = false;
            if (WS_GATHER_TEST == 2 && ((b >> 6) & 1) && lane == 5) ok2 = false;
#endif
            if (__ballot(!(ok1 && ok2))) { v1 = slow(e1, a1); v2 = slow(e2, a2); WS_STAT(d, 3, 1); }
            if (a1) accv += v1;
            if (two && a2) accv += v2;
        }
        if (in) L.oE[i] = accv;
        if (hpPark && b < (kFirst + jB - jA + 1) * g.C) {
            iir_block_park((const lds_f64 *)L.oE, L.yF, b, hpPark);
#ifdef VP_STAMPS
            { const struct { int nChunk0; } c = {nChunk0}; if (m == 0) WS_EV(d, 13, 7); }   // (the parked segment's first block is parked)
#endif
        }
        WS_STAT(d, 0, 1); WS_STAT(d, 1, WS_CLK() - tTrip0);
        // done: the trip's instance counts it; its last one releases the instance
        int r = 0;
        for (int q = 1; q <= jB - jA; q++) r += (b >= (kFirst + q) * g.C) ? 1 : 0;
        __threadfence_block();
        int was = 0;
        if (lane == 0) was = __hip_atomic_fetch_add((lds_i32 *)&ctl->gDone[jA + r], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        was = __builtin_amdgcn_readfirstlane(was);
        if (was + 1 == count(r)) release(jA + r);
    }
}

// ------------------------------------------------------------------------------------------------
// BACKGROUND program: everything PitchProcess::processChunkStart (PitchProcess.cpp:203-233) does before the residual, for the
// block's frame starts in order, on the private state copy stBG.  bw = 0..3: the background wavefront's rank; rank 3 LEADS
// (combines the transforms, picks, places the marks, publishes); rank 0 takes the prefix sums, ranks 1 and 2 the LPC chain.
// BIG (round 6, the _o24 builds): lpcPitch 16 .. WS_ORDER_MAX -- the phase kernels' forms for those orders (two groups of sixteen lags
// on the two LPC wavefronts, levinson_fast64 / levinson_row48, 128 samples of impulse response, the block recursion with a history
// matrix / the one-lane exact chain); the builds for lpcPitch <= 15 carry none of it.
template <bool FAST, bool BIG, bool LEAN = false>
__device__ __forceinline__ void ws_background(const VpGeom &g0, const VpCall &c, const VpDev &d, const VpWsSched &sc, lds_f64 *sm, const WsCarve &cv0,
                                              lds_ctl *ctl, int bw, int gateOpen)
{
    lds_state *stBG = (lds_state *)(sm + cv0.st) + 1;
    const bool lead = bw == WS_NBG - 1;
    int bgBarGen = 0;
    PitchLds L;
    L.qtab = nullptr; L.htab = nullptr;
    L.st = stBG;
    L.ishare = (int *)ctl->ishareBG;          // (the shared routines take it as a generic pointer)
    L.fftFlag = (int *)ctl->fftFlag;
    L.xcA = nullptr;
    L.oA = nullptr; L.pend = nullptr;
    L.gateOpen = gateOpen;
    const int wq = (int)(blockDim.x / WAVE) - WS_NBG + bw;   // (the wavefront's index, for the diagnostic timers)
    (void)wq;
    const int nStart = sc.nStart;
    for (int i = 0; i < nStart; i++) {
        const int gen = i + 1;
        // (the geometry through opaque moves once per start: what is derived from it -- dozens of loop bounds, predicates and offsets of
        // every path below, taken or not -- was otherwise computed in front of this loop, 550 scalar instructions and their spills to
        // vector lanes at the head of the start's critical chain)
        VpGeom g = g0;
        WsCarve cv = cv0;
        // (LEAN: all but tau0 are constants of the build -- nothing derived from them is computed at all)
        if constexpr (LEAN) asm volatile("" : "+s"(g.tau0));
        else
        asm volatile("" : "+s"(g.tauMax), "+s"(g.F), "+s"(g.C), "+s"(g.toKeep), "+s"(g.orderPitch), "+s"(g.tau0));
        asm volatile("" : "+s"(cv.xs), "+s"(cv.fr), "+s"(cv.P), "+s"(cv.dY), "+s"(cv.r), "+s"(cv.aPrev), "+s"(cv.hp), "+s"(cv.xp), "+s"(cv.aF), "+s"(cv.tw));
        L.eF = sm + cv.P;                              // the prefix sums live where the phase kernel parks them: "eFrame"
        L.cum = sm + cv.P;                             // (the fallback's running sum: the prefix sums are dead by then)
        L.dY = sm + cv.dY;
        L.fftTw = (lds_d2 *)(sm + cv.tw);
        if (lead) WS_FINE(d, 0);
        // (the lane index through the opaque move once per start: what is derived from it must not be hoisted out of this loop -- the
        // fallback's sixteen multipliers and the prefix sums' masks were, and lived in scratch across the whole program)
        const int lane = vp_tid() & 63;
        if (!gateOpen) {                                                      // :208-214
            if (lead) {
                ws_wait_ge<LEAN>(&ctl->bgAdopt, i, d);                            // (the producers adopt the state straight from this copy: they are done with the previous start's)
                if (lane == 0) { stBG->nAn = 0; stBG->prevPitch = 0; stBG->gateOpen = 0; ctl->pubMode = 0; }
                ws_signal(&ctl->bgPub, gen);
            }
            continue;
        }
        const int pn = sc.startPar[i], tS = sc.startStep[i];
        // the frame's parity buffers (and with them the exchange buffers) are free once the previous frame of that parity has
        // had its last chunk's recursion and output
        ws_wait_ge<LEAN>(&ctl->fillTurn, sc.startNeed[i], d);
        if (i == 0) WS_EV(d, wq, 0);
        L.xs = sm + cv.xs + ((g.toKeep - g.tauMax) & 1) + tS * g.C;
        L.r = sm + cv.r + pn * 64;                     // (per parity: a wavefront may be a start ahead of the one that reads these)
        L.aPrev = sm + cv.aPrev + pn * (VP_ORDER_MAX + 2);
        lds_f64 *frBase = sm + cv.fr;
        lds_f64 *oEn = pn ? frBase + 3 * g.F + 2048 : frBase, *yFn = pn ? frBase + 2 * g.F + 2048 : frBase + g.F;
        L.oE = oEn; L.yF = yFn;
        L.fftBuf = (lds_d2 *)(pn ? frBase + 2 * g.F : frBase);
        const int base = g.toKeep - g.tauMax;
        const lds_f64 *xw = L.xs + base, *xf = L.xs + g.toKeep;
        const int xcCert = c.yinCert;
        // ---- the certified form's cross-correlations: one forward transform per wavefront, the lead combines (xcorr_fft_wave)
        // (at a raised issue priority: the start's critical chain begins with these transforms, and three wavefronts share every SIMD)
        VP_PRIO_UP();
        if (xcCert) xcorr_fft_wave(g, d, L, xw, lead ? 0 : bw + 1, WS_NBG, gen);
        VP_PRIO_DOWN();
        if (i == 0) WS_EV(d, wq, 1);                                          // transforms done (lead: cross-correlations in yinTemp)
        if (bw == 0) {
            if (xcCert) { ws_prefix_sums(xw, L.eF, g.F + g.tauMax); ws_signal(&ctl->pDone, gen); }
            if (i == 0) WS_EV(d, wq, 2);
        } else if (bw == 1) {
            // ---- LPC autocorrelation of the frame (LPC.cpp:44-97), second half of the sums (FAST) / lags 0..7 (EXACT)
            if (BIG) {
                // (orders 16 ..: FAST: the groups of sixteen lags 1, 3, ...; EXACT: the passes of eight lags from 8, 24, ... -- as the phase
                // kernels deal them to their two LPC wavefronts, vp_pitch.inc lpcTwo / acRows: same routines, same bits)
                if (FAST) autocorr_rows_fast<true, false>(xf, g.F, g.orderPitch, L.r, 1, 2);
                else for (int lag0 = 8; lag0 <= g.orderPitch; lag0 += 16) autocorr_rows_exact8(xf, g.F, g.orderPitch, lag0, L.r);
            } else
            if (FAST) {
                const double t1 = autocorr_rows_fast_half<true>(xf, g.F, 1);
                if (lane < 16) L.r[32 + lane] = t1;
            } else
                autocorr_rows_exact8(xf, g.F, g.orderPitch, 0, L.r);
            ws_signal(&ctl->acDone, gen);
            if (i == 0) WS_EV(d, wq, 2);
        } else if (bw == 2) {
            VP_PRIO_UP();
            const int order = g.orderPitch;
            if (BIG) {
                if (FAST) autocorr_rows_fast<true, false>(xf, g.F, order, L.r, 0, 2);
                else for (int lag0 = 0; lag0 <= order; lag0 += 16) autocorr_rows_exact8(xf, g.F, order, lag0, L.r);
                ws_wait_ge<LEAN>(&ctl->acDone, gen, d);
            } else
            if (FAST) {
                const double t0 = autocorr_rows_fast_half<true>(xf, g.F, 0);
                ws_wait_ge<LEAN>(&ctl->acDone, gen, d);
                const double t1 = L.r[32 + (lane & 15)];
                if (lane < 16 && lane <= order) L.r[lane] = (t0 + t1) / vp_f64_here(g.F);
            } else {
                if (order >= 8) autocorr_rows_exact8(xf, g.F, order, 8, L.r);
                ws_wait_ge<LEAN>(&ctl->acDone, gen, d);
            }
            // levinsonDurbin (LPC.cpp:107-148), then the impulse response of 1/A(z) for the block-form recursion, the frame's
            // coefficients where the recursion wavefronts read them
            if (i == 0) WS_EV(d, wq, 2);                                      // autocorrelation complete
            const bool z = !BIG ? levinson_row16(L.r, L.aPrev, order, VP_ORDER_MAX + 1, g.levEps)
                           : FAST ? levinson_fast64(L.r, L.aPrev, order, VP_ORDER_MAX + 1, g.levEps)
                                  : levinson_row48(L.r, L.aPrev, order, VP_ORDER_MAX + 1, g.levEps);
            if (i == 0) WS_EV(d, wq, 3);
            lds_f64 *hpad = sm + cv.hp + pn * WS_HP(g), *xp = sm + cv.xp, *aFn = sm + cv.aF + pn * WS_AF(g);
            hpad[lane] = 0.0;
            xp[lane] = (lane == 0) ? 1.0 : 0.0;
            // (orders above 16: the block recursion with a history matrix takes 128 samples of the response, vp_pitch.inc pitch_impulse_response)
            const int nh = (BIG && order > 16) ? 2 * WAVE : WAVE;
            if (BIG) xp[WAVE + lane] = 0.0;
            iir_fast_wave(xp, hpad + WAVE, nh, (const lds_f64 *)L.aPrev, order, (const lds_f64 *)nullptr, 1.0);
            if (lane < WS_AF(g)) aFn[lane] = (lane <= order) ? L.aPrev[lane] : 0.0;
            if (lane == 0) ctl->lpcZ[pn] = z ? 1 : 0;
            ws_signal(&ctl->lpcDone, gen);
            if (i == 0) WS_EV(d, wq, 4);
            VP_PRIO_DOWN();
        }
        // ---- yin() to the end, on the lead
        if (lead) {
            VP_PRIO_UP();
            int fallback = 1;
            // yin()'s state roll (:415-425) -- here, not at the top: the producers adopt a published start straight from this copy, and
            // by now they have long done so (nothing before this point touches the state)
            ws_wait_ge<LEAN>(&ctl->bgAdopt, i, d);
            if (lane == 0) {
                stBG->gateOpen = 1;
                stBG->prevPeriod = stBG->period;
                stBG->prevPitch = stBG->pitch;
                if (stBG->pitch > 1) { stBG->prevVoicedPeriod = stBG->period; stBG->prevVoicedPitch = stBG->pitch; }
                stBG->pitch = 0; stBG->period = 0;
                ctl->ishareBG[0] = INT_MAX;
                ctl->ishareBG[1] = 0;
            }
            wave_sync();
            WS_FINE(d, 1);
            if (xcCert) {
                ws_wait_ge<LEAN>(&ctl->pDone, gen, d);
                if (i == 0) WS_EV(d, wq, 2);
                xc_scan_pick(g, L, stBG, xcCert, true);
                wave_sync();
                fallback = ctl->ishareBG[1] != 0;
                if (lane == 0) atomicAdd(&d.dbg[fallback ? 63 : 62], 1ULL);
                ws_signal(&ctl->xcDone, gen);                                 // the exchange buffers are free
                if (!fallback) {                                              // the grain half-length is final: the producers may stage the Hann window
                    if (lane == 0) ctl->pickT[pn] = (stBG->pitch > 1) ? stBG->period : stBG->prevVoicedPeriod;
                    ws_signal(&ctl->tDone, gen);
                }
            }
            if (lane == 0) ctl->pickState = fallback;
            ws_signal(&ctl->pickDone, gen);
            if (i == 0) WS_EV(d, wq, 3);
            VP_PRIO_DOWN();
        }
        ws_wait_ge<LEAN>(&ctl->pickDone, gen, d);                                 // (no helping here: trips beside the lead's pick and marks slow the start's chain down)
        if (ctl->pickState) {
            // a comparison of the certified form was too close to call (or VP_YIN_DIRECT): the frame's difference function in
            // the reference's arithmetic, two adjacent lags per lane on the four wavefronts, its running sum and pick on the lead
            if (lead && lane == 0) { ctl->ishareBG[0] = INT_MAX; ctl->ishareBG[1] = 0; }
            yin2_exact_waves(g, L, base, bw * WAVE + (vp_tid() & 63), 0, WS_NBG, (g.tauMax + 1) >> 1);
            ws_group_barrier<LEAN>(&ctl->bgBar, WS_NBG, bgBarGen, d);
            if (lead) {
                yin_cumsum_wave(g, L, vp_tid() & 63);
                wave_sync();
                ws_yin_pick_wave(g, d, L, stBG);
                wave_sync();
                if ((vp_tid() & 63) == 0) ctl->pickT[pn] = (stBG->pitch > 1) ? stBG->period : stBG->prevVoicedPeriod;
                ws_signal(&ctl->tDone, gen);
            }
            ws_group_barrier<LEAN>(&ctl->bgBar, WS_NBG, bgBarGen, d);           // (the running sum lives where the next start's prefix sums go)
        }
        // :216-218 for the coming frame: its outEFrame and yFrame start from zero (the exchange buffers lived there)
        if (!lead) {
            if (xcCert) ws_wait_ge<LEAN>(&ctl->xcDone, gen, d);
            for (int q = bw * WAVE + lane; q < g.F; q += (WS_NBG - 1) * WAVE) { oEn[q] = 0.0; yFn[q] = 0.0; }
            __threadfence_block();
            if (lane == 0) __hip_atomic_fetch_add((lds_i32 *)&ctl->zeroDone, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            continue;
        }
        // ---- pitchMarks, placeStMarks (:224-227) on the lead
        VP_PRIO_UP();
        {
            const int key = stBG->sp.key;
            const NoteRegs nr = notes_request(d.notes + (size_t)key * VP_NOTES_STRIDE);
            const int notesN = d.notesN[key];
            WS_FINE(d, 2);
            pitch_marks(g, L, d.ub);
            WS_FINE(d, 3);
            place_st_marks(g, c, d, stBG, nr, notesN);
        }
        wave_sync();
        if (i == 0) WS_EV(d, wq, 4);                                          // marks placed
        ws_wait_ge<LEAN>(&ctl->lpcDone, gen, d);
        if (stBG->nAn != 0) {                                                 // the coefficients are adopted (:233)
            const int ncopy = ctl->lpcZ[pn] ? VP_ORDER_MAX + 1 : g.orderPitch + 1;
            for (int q = lane; q < ncopy; q += WAVE) stBG->a[q] = L.aPrev[q];
        }
        WS_FINE(d, 4);
        ws_wait_ge<LEAN>(&ctl->zeroDone, (WS_NBG - 1) * gen, d);
        WS_FINE(d, 5);
        if (lane == 0) ctl->pubMode = stBG->nAn != 0 ? 2 : 1;
        ws_signal(&ctl->bgPub, gen);
        WS_EV(d, wq, i == 0 ? 5 : 6);                                         // published (second start: slot 6)
        VP_PRIO_DOWN();
    }
}

// ------------------------------------------------------------------------------------------------
// PRODUCER program: the block's SEGMENTS in order (a segment = the chunks of one frame that this block's steps run), everything of
// a chunk that does not depend on the recursion: the residual (filterFIR :280-302), the quotient / Hann tables of the frame, the
// grain table and the gather pass of psola() (:665-741).  rank 0 owns the serial part (the table); the group meets at its own barrier.
template <bool FAST, bool LEAN = false>
__device__ __forceinline__ void ws_producer(const VpGeom &g, const VpCall &c, const VpDev &d, const VpWsSched &sc, lds_f64 *sm, const WsCarve &cv,
                                            lds_ctl *ctl, int rank, int nP, int gateOpen, bool firstBlock = true, bool lastBlock = true)
{
    const int lane = vp_tid() & 63, tp = rank * WAVE + lane, ntp = nP * WAVE;
    lds_state *st = (lds_state *)(sm + cv.st), *stPub = st + 1;            // (the background's own copy IS the published one)
    lds_f64 *xsAll = sm + cv.xs + ((g.toKeep - g.tauMax) & 1);
    lds_f64 *frBase = sm + cv.fr;
    int barGen = 0;
    bool qValid = false;
    PitchLds L;
    L.st = st;
    L.eF = sm + cv.eF;
    L.qtab = sm + cv.qtab;
    L.htab = sm + cv.htab;
    const SegTab G = ws_seg_tab(sm + cv.gtab);
    const int order = g.orderPitch;
    const int wq = rank + 2;
    (void)wq;
    WS_EV(d, wq, 0);
    WS_TB();
    const int s_ = vp_stream(d);
    if (firstBlock && c.nChunk0 != 0 && st->nAn != 0) {                      // (later blocks of a multi-block launch: it never left the LDS)
        // the frame in flight: its residual up to where the previous block left it (this block's first segment computes on from
        // there and zeroes the rest).  Requested here, not in the prologue: 22 KB per stream that only this group reads, and it
        // has time -- the recursion and the background start without it (in the prologue it cost the background's chain 0.7 us).
        const double *ge = d.eFrame + (size_t)s_ * g.eLen;
        const int lim = min(g.eLen, g.toKeep + g.F + (c.nChunk0 - 1) * g.C);
        for (int q = tp; q < lim; q += ntp) L.eF[q] = ge[q];
    }
    for (int sg = 0; sg < sc.nSeg; sg++) {
        const int jA = sc.segA[sg], jB = sc.segB[sg];
        const int t = sc.instStep[jA], kFirst = sc.instK[jA], kLast = sc.instK[jB], p = sc.instPar[jA], si = sc.instStart[jA];
        const int pS = c.pStart + t * g.C;
        // (FAST, orders up to 16 -- iir_block_wave_regs' path --: the segments the schedule names park the recursion's first pass)
        const bool park = FAST && order <= 16 && sc.segPark[sg] != 0;
        const lds_f64 *hpPark = park ? (const lds_f64 *)(sm + cv.hp + p * WS_HP(g)) : (const lds_f64 *)nullptr;
        WS_TR();
        L.xs = xsAll + t * g.C;
        L.oE = p ? frBase + 3 * g.F + 2048 : frBase;
        L.yF = p ? frBase + 2 * g.F + 2048 : frBase + g.F;
        int mode;
        if (si >= 0) {
            // processChunkStart.  What needs only the new coefficients or the grain half-length is done while the background still
            // places the marks: filterFIR(-toKeep, toKeep+F, 0) :235 -- and, in the same pass, the residual of the frame's Cont
            // chunks inside this block (:258-259): in eFrame's coordinates they simply continue the frame's (eFrame index = index into
            // the Start step's voice window); what lies beyond starts from zero (:216); the gather reads entries a chunk has not
            // "computed yet" as zero (SegTab::eLim) -- and the frame's Hann window (fillPsolaWindow :878-882).  Speculative like the
            // phase kernel's: a frame without analysis marks zeroes eFrame again.
            const int jEnd = g.toKeep + g.F + (jB - jA) * g.C;
            if (gateOpen && rank != 0) {                                      // (rank 0 keeps itself free for the tables: the serial part)
                ws_wait_ge<LEAN>(&ctl->lpcDone, si + 1, d);
                WS_TA(d, wq, 1);
                const lds_f64 *aN = sm + cv.aF + p * WS_AF(g);
                for (int q = 4 * (tp - WAVE); q < jEnd; q += 4 * (ntp - WAVE)) fir4((const lds_f64 *)L.xs, aN, order, q, jEnd, L.eF);
                for (int q = jEnd + tp - WAVE; q < g.eLen; q += ntp - WAVE) L.eF[q] = 0.0;
                WS_TA(d, wq, 2);
                ws_wait_ge<LEAN>(&ctl->tDone, si + 1, d);
                WS_TA(d, wq, 1);
                const int T = ctl->pickT[p];
                const double *hg = d.hannTab + d.hannOff[T];
                for (int q = tp - WAVE; q < 2 * T + 1; q += ntp - WAVE) L.htab[q] = hg[q];
                WS_TA(d, wq, 2);
            }
            // the background has the new frame's pitch, marks and coefficients ready (or is about to)
            ws_wait_ge<LEAN>(&ctl->bgPub, si + 1, d);
            WS_TA(d, wq, 1);                                                  // waited for the background
            WS_FINEP(d, 0);
            mode = ctl->pubMode;
            if (rank == 0) {
                // rank 0 goes straight to the segment's grain table, from the published copy of the tracker state (the chunk progress,
                // stMarkIdx, is this group's own) ...
                if (mode == 2) {
                    if (lane == 0) st->stMarkIdx = 0;                         // :238
                    wave_sync();
                    ws_psola_table_seg(g, d, stPub, st, G, kFirst, kLast, pS, ctl, sg, park);
                }
                WS_TA(d, wq, 4);                                              // grain table
                WS_FINEP(d, 2);
            } else {
                if (rank == 1) {
                    // ... which rank 1 meanwhile adopts for the group ...
                    const int keep = (int)(offsetof(VpPitchState, stMarkIdx) / sizeof(int));
                    const lds_i32 *src = (const lds_i32 *)stPub;
                    lds_i32 *dst = (lds_i32 *)st;
                    for (int q = lane; q < (int)(sizeof(VpPitchState) / sizeof(int)); q += WAVE) if (q != keep) dst[q] = src[q];
                    WS_FINEP(d, 1);
                }
                if (mode == 2) {
                    // ... and everybody but rank 0 fills the frame's quotient table: xInterp[j] - stMark = (j - T) / beta is the same for
                    // every grain of the frame (:700,715,731)
                    const int T = (stPub->pitch > 1) ? stPub->period : stPub->prevVoicedPeriod;
                    const double beta = stPub->beta;
                    for (int q = tp - WAVE; q < 2 * T + 1; q += ntp - WAVE) L.qtab[q] = (double)(q - T) / beta;
                }
                WS_TA(d, wq, 2);
                WS_FINEP(d, 2);
            }
            if (mode == 1) for (int q = tp; q < jEnd; q += ntp) L.eF[q] = 0.0;   // no analysis marks: the frame stays as :216-218 left it
            qValid = mode == 2;
            ws_group_barrier<LEAN>(&ctl->prodBar, nP, barGen, d);
            WS_TA(d, wq, 3);
            WS_FINEP(d, 3);
            if (rank == 0) ws_signal(&ctl->bgAdopt, si + 1);                  // (everybody has read the published copy)
        } else {
            // processChunkCont (:253-271) of the frame in flight: only if analysis marks exist
            mode = (st->nAn != 0) ? 2 : 0;
            if (mode == 2) {
                if (rank == 0) {
                    ws_psola_table_seg(g, d, st, st, G, kFirst, kLast, pS, ctl, sg, park);
                    WS_TA(d, wq, 4);
                } else {
                    // filterFIR(F-C, C, ...) :258-259 of the segment's chunks (what lies beyond: nothing there yet, :216) and, once per
                    // frame and launch, the quotient / Hann tables (:700,715,731; fillPsolaWindow :878-882)
                    const int j0 = g.toKeep + g.F - g.C, jEnd = j0 + (jB - jA + 1) * g.C;
                    for (int q = j0 + 4 * (tp - WAVE); q < jEnd; q += 4 * (ntp - WAVE)) fir4((const lds_f64 *)L.xs, (const lds_f64 *)st->a, order, q, jEnd, L.eF + kFirst * g.C);
                    for (int q = kFirst * g.C + jEnd + tp - WAVE; q < g.eLen; q += ntp - WAVE) L.eF[q] = 0.0;
                    if (!qValid) {
                        const int T = (st->pitch > 1) ? st->period : st->prevVoicedPeriod;
                        const double beta = st->beta;
                        const double *hg = d.hannTab + d.hannOff[T];
                        for (int q = tp - WAVE; q < 2 * T + 1; q += ntp - WAVE) { L.qtab[q] = (double)(q - T) / beta; L.htab[q] = hg[q]; }
                    }
                    WS_TA(d, wq, 2);
                }
                qValid = true;
                ws_group_barrier<LEAN>(&ctl->prodBar, nP, barGen, d);
                WS_TA(d, wq, 3);
            }
        }
        if (mode == 2) {
            // the gather pass; the segment is over -- its tables, the residual and the quotient / Hann tables free for the next one's --
            // when its last instance is out
            ws_psola_gather_seg<LEAN>(g, d, L, G, ctl, sg, jA, jB, kFirst, rank == 0, hpPark, c.nChunk0);
            WS_FINEP(d, 4);
            WS_TA(d, wq, 5);                                                  // gather pass
            ws_wait_ge<LEAN>(&ctl->psDone, jB + 1, d);
            WS_FINEP(d, 6);
            WS_TA(d, wq, 3);
        } else {
            ws_group_barrier<LEAN>(&ctl->prodBar, nP, barGen, d);
            WS_TA(d, wq, 3);
            if (rank == 0) {
                // a Start decides for its frame (no marks: output only, and the Cont chunks do nothing, :255)
                if (lane <= jB - jA) ctl->instMode[jA + lane] = (lane == 0) ? mode : 0;
                ws_signal(&ctl->psDone, jB + 1);
            }
        }
    }
    {   // the frame in flight at the end of the block goes back to HBM from here -- the residual is this group's own -- while the
        // recursion still runs (the epilogue writes the rest: state, outEFrame, yFrame, impulse response)
        int nChunkEnd = c.nChunk0;
        for (int t = 0; t < c.nSteps; t++) { if (nChunkEnd == g.cpf - 1) nChunkEnd = 0; nChunkEnd += 1; }
        if (lastBlock && nChunkEnd != 0 && st->nAn != 0) {
            double *ge = d.eFrame + (size_t)s_ * g.eLen;
            for (int q = tp; q < g.eLen; q += ntp) ge[q] = L.eF[q];
        }
    }
    WS_EV(d, wq, 7);
}

// ------------------------------------------------------------------------------------------------
// RECURSION program: filterIIR (PitchProcess.cpp:307-322) and fillOutputBuffer (:328-342) of the instances, by ONE wavefront
// (EXACT: two, frames alternating -- the reference's chain is one dependent sequence per frame, 25 us per chunk, and two
// consecutive frames share nothing).  The additions into the output keep the reference's order through fillTurn.
template <bool FAST, bool BIG, bool LEAN = false>
__device__ __forceinline__ void ws_recursion(const VpGeom &g, const VpCall &c, const VpDev &d, const VpWsSched &sc, lds_f64 *sm, const WsCarve &cv,
                                             lds_ctl *ctl, int me, int nIir, double gainPitch)
{
    const int nInst = sc.nInst;
    const int lane = vp_tid() & 63;
    lds_f64 *frBase = sm + cv.fr, *oA = sm + cv.oA;
    const int order = g.orderPitch;
    const int nW = g.C / WAVE;                                               // (common case: the chunk is a multiple of 64 samples, at most 512)
    VP_PRIO_UP();
    WS_EV(d, me, 0);
    WS_TB();
    // fillOutputBuffer (:328-342) of instance j: yFrame * stWindow * gain, added where the block's accumulator slice lives
    auto fill = [&](int j, const double (&win)[8]) {
        const int p = sc.instPar[j], pS = c.pStart + sc.instStep[j] * g.C, shift = sc.instK[j] * g.C;
        const lds_f64 *yF = p ? frBase + 2 * g.F + 2048 : frBase + g.F;
        if (ctl->instMode[j] >= 1) {
#pragma unroll
            for (int u = 0; u < 8; u++) if (u < nW) {
                const int i = lane + WAVE * u;
                oA[pS + i] += yF[shift + i] * win[u] * gainPitch;
            }
        }
        ws_signal(&ctl->fillTurn, j + 1);
    };
    auto window = [&](int j, double (&win)[8]) {
        const int shift = sc.instK[j] * g.C;
#pragma unroll
        for (int u = 0; u < 8; u++) win[u] = (u < nW) ? d.pitchStWin[shift + lane + WAVE * u] : 0.0;
    };
    // EXACT (two recursion wavefronts): a finished chunk whose turn to add has not come -- the other frame's chunk before it is
    // still in its 20 us chain -- does not hold up this frame's next chunk: its addition waits in line (fj: my first unfilled one)
    int fj = 0;
    auto flush = [&](int upto, bool block) {
        for (; fj < upto; fj++) {
            if (sc.instPar[fj] != me) continue;
            if (!block && __hip_atomic_load(&ctl->fillTurn, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < fj) break;
            ws_wait_ge<LEAN>(&ctl->fillTurn, fj, d);
            double win[8];
            window(fj, win);
            fill(fj, win);
        }
    };
    // FAST, orders up to 16: the instances of the segments whose producers park the routine's first pass (VpWsSched::segPark: a suffix
    // of the block's segments) are the second loop's; everything else takes the one-piece routine as before
    int jPark = nInst;
    if (FAST && order <= 16) for (int sg = sc.nSeg - 1; sg >= 0 && sc.segPark[sg] != 0; sg--) jPark = sc.segA[sg];
    for (int j = 0; j < jPark; j++) {
        const int p = sc.instPar[j];
        if (nIir > 1 && p != me) continue;
        WS_TR();
        const int k = sc.instK[j], shift = k * g.C;
        lds_f64 *oE = p ? frBase + 3 * g.F + 2048 : frBase, *yF = p ? frBase + 2 * g.F + 2048 : frBase + g.F;
        const lds_f64 *aF = sm + cv.aF + p * WS_AF(g), *hpad = sm + cv.hp + p * WS_HP(g);
        if (!FAST && nIir > 1) {
            // EXACT, two recursion wavefronts: while this one waits for its next chunk, it keeps adding the chunks it has finished
            // as their turns come.  Blocked in a plain wait it could hold the unflushed additions of frame P while frame R's Start
            // -- which must see all of P added before it may reuse P's parity buffers (startNeed) -- never publishes R's chunks:
            // a circular wait (blocks of 2 cpf - 1 steps and more, one wavefront a whole frame behind the other).
            int spin = 0;
            while (__hip_atomic_load(&ctl->psDone, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < j + 1) {
                flush(j, false);
                if (++spin >= d.spinLimit) {
                    if constexpr (LEAN) ws_lean_tmo[0] = 1;                   // (EXACT only: no LEAN build reaches this; kept in step with ws_wait_ge)
                    else if (lane == 0) vp_timeout(vp_tmo(d, 61));
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        } else
        ws_wait_ge<LEAN>(&ctl->psDone, j + 1, d);
        WS_TA(d, me, 1);                                                      // waited for the producers
        if (me == 0) WS_FINER(d, j);
        const int mode = ctl->instMode[j];
        if (mode == 2) {
            if (FAST)
                // (the routine's first pass -- two thirds of its terms need no earlier output -- on the wavefront beside this one as soon
                // as a chunk is released, the second here: measured, no gain: 2.0 + 1.7 us per chunk in a pipeline against 2.6 here)
            {
                // (orders above 16: zero-state responses + history matrix, as vp_k_pitch_fast's pitch_iir_wave takes them -- same sums)
                if (BIG && order > 16) iir_block_wave_hc<32>((const lds_f64 *)(oE + shift), yF + shift, g.C, aF, order, min(order, shift), hpad, 1.0);
                else iir_block_wave_regs((const lds_f64 *)(oE + shift), yF + shift, g.C, aF, order, shift > 0, hpad);
            } else {
                lds_f64 *hist = sm + cv.hist + me * WS_HIST(g);
                const int nh = min(order, shift);
                for (int q = 0; q < order; q++) hist[q] = (q < nh) ? yF[shift - 1 - q] : 0.0;
                if (BIG && order > 16) iir_exact_lane<24>((const lds_f64 *)(oE + shift), yF + shift, g.C, aF, order, (const lds_f64 *)hist, 1.0);
                else iir_exact_row16((const lds_f64 *)(oE + shift), yF + shift, g.C, aF, order, (const lds_f64 *)hist, 1.0);
            }
        }
        WS_TA(d, me, 2);                                                      // recursion
        if (FAST)
            ws_signal(&ctl->iirDone, j + 1);                                  // (the windowed add is the next wavefront's: ws_filler)
        else
            flush(j + 1, false);
        WS_TA(d, me, 4);                                                      // windowed add
    }
    if constexpr (FAST) {
        // The parked instances: their blocks' first-pass sums lie in yFrame when the producers release them (instMode 3), so what is
        // left on this chain is the walk.  Its 64 registers of taps and history coefficients are the FRAME's: a Cont instance has them
        // before the wait -- kept from the chunk before, or requested while the producers are still at work (the frame in flight's
        // lie in LDS since the prologue) -- instead of 80 LDS values requested behind it; a Start's are final only with its release.
        IirWalkRegs R;
        bool haveR = false;
        for (int j = jPark; j < nInst; j++) {
            const int p = sc.instPar[j];
            WS_TR();
            const int k = sc.instK[j], shift = k * g.C;
            lds_f64 *oE = p ? frBase + 3 * g.F + 2048 : frBase, *yF = p ? frBase + 2 * g.F + 2048 : frBase + g.F;
            const lds_f64 *aF = sm + cv.aF + p * WS_AF(g), *hpad = sm + cv.hp + p * WS_HP(g);
            if (sc.instStart[j] >= 0) haveR = false;
            else if (!haveR) { iir_block_walk_load(R, aF, order, hpad); haveR = true; }
            ws_wait_ge<LEAN>(&ctl->psDone, j + 1, d);
            WS_TA(d, me, 1);                                                  // waited for the producers
            WS_FINER(d, j);
            if (ctl->instMode[j] == 3) {
                if (!haveR) { iir_block_walk_load(R, aF, order, hpad); haveR = true; }
                if (j == jPark) WS_EV(d, 14, 7);                              // (diagnostic: the first parked instance's walk starts)
                iir_block_walk(R, (const lds_f64 *)(oE + shift), yF + shift, g.C, order, shift > 0);
            }
            WS_TA(d, me, 2);                                                  // recursion
            ws_signal(&ctl->iirDone, j + 1);
            WS_TA(d, me, 4);
        }
    }
    if (!FAST) { WS_TR(); flush(nInst, true); WS_TA(d, me, 3); }
    WS_EV(d, me, me == 0 ? 6 : 7);
    VP_PRIO_DOWN();
}

// FAST: fillOutputBuffer (:328-342) of the instances on a wavefront of its own, in the reference's order, right behind the recursion
// (which then goes straight on to its next chunk)
template <bool LEAN = false>
__device__ __forceinline__ void ws_filler(const VpGeom &g, const VpCall &c, const VpDev &d, const VpWsSched &sc, lds_f64 *sm, const WsCarve &cv,
                                          lds_ctl *ctl, double gainPitch)
{
    const int lane = vp_tid() & 63;
    lds_f64 *frBase = sm + cv.fr, *oA = sm + cv.oA;
    const int nW = g.C / WAVE;
    VP_PRIO_UP();
    for (int j = 0; j < sc.nInst; j++) {
        const int p = sc.instPar[j], pS = c.pStart + sc.instStep[j] * g.C, shift = sc.instK[j] * g.C;
        const lds_f64 *yF = p ? frBase + 2 * g.F + 2048 : frBase + g.F;
        double win[8];
#pragma unroll
        for (int u = 0; u < 8; u++) win[u] = (u < nW) ? d.pitchStWin[shift + lane + WAVE * u] : 0.0;   // requested before the wait
        ws_wait_ge<LEAN>(&ctl->iirDone, j + 1, d);
        if (ctl->instMode[j] >= 1) {
#pragma unroll
            for (int u = 0; u < 8; u++) if (u < nW) {
                const int i = lane + WAVE * u;
                oA[pS + i] += yF[shift + i] * win[u] * gainPitch;
            }
        }
        ws_signal(&ctl->fillTurn, j + 1);
    }
    VP_PRIO_DOWN();
}

// emit_block (vp_kernels.hip: addDryVoice / addSynth MyBuffer.cpp:309-448, fillOutputBuffer + clearOutput :113-133, 218-228) from the
// accumulator slice in LDS, ring positions by conditional subtraction (counter < size, i < N <= size) instead of a run-time modulo
__device__ __forceinline__ void ws_emit_block(const VpGeom &g, const VpCall &c, const VpDev &d, float *__restrict__ out, const lds_state *stl,
                                              const lds_f64 *oA)
{
    const int s = vp_stream(d);
    const float *vr = d.voiceRing + (size_t)s * g.inSize;
    const float *sr0 = d.synthRing + (size_t)s * 2 * g.inSize;
    const float *sr1 = sr0 + g.inSize;
    double *acc = d.outAcc + (size_t)s * g.outSize;
    double *acc2 = d.outAcc2 ? d.outAcc2 + (size_t)s * g.outSize : nullptr;
    float *o = out + (size_t)s * (c.inplace ? 3 : 2) * g.N;
    const int dryOn = stl->sp.dryOn, synthOn = stl->sp.synthOn;
    const double gainVoice = stl->sp.gainVoice, gainSynth = stl->sp.gainSynth;
    // (one sample per lane and trip: with four -- a quarter of the load and store instructions, but a third of the wavefronts at work --
    // the block was 0.4 us LONGER, measured; the prologue's requests are the opposite case)
    for (int i = vp_tid(); i < g.N; i += blockDim.x) {
        int pos = c.outCounter + i, pin = c.currCounter + i;
        pos -= (pos >= g.outSize) ? g.outSize : 0;
        pin -= (pin >= g.inSize) ? g.inSize : 0;
        double v = oA[i];
        if (acc2) { v += acc2[pos]; acc2[pos] = 0.0; }                       // the pitch corrector's share, when it ran beside the vocoder
        if (dryOn) v += (double)vr[pin] * gainVoice;
        double l = v, r = v;
        if (synthOn) { l += (double)sr0[pin] * gainSynth; r += (double)sr1[pin] * gainSynth; }
        o[i] = (float)l;
        o[g.N + i] = (float)r;
        if (c.inplace) o[2 * g.N + i] = 0.0f;
        acc[pos] = 0.0;
    }
}

// ---- several queued blocks per launch (round 6): what stands between two blocks of vp_k_pitch_ws_mb -----------------------------------
// Everything the programs derive from the kernel's arguments must stay INSIDE the block loop: laundered through empty asm statements
// per block, the values are opaque to the compiler, so nothing computed from them is hoisted in front of the loop and carried in
// registers across all four programs (round 5's attempt at this loop: 340 spilled registers, 51 us per block).
__device__ __forceinline__ void ws_mb_launder(VpGeom &g, VpCall &c, VpDev &d)
{
    asm volatile("" : "+s"(g.S), "+s"(g.N), "+s"(g.F), "+s"(g.H), "+s"(g.C), "+s"(g.cpf), "+s"(g.toKeep), "+s"(g.latency), "+s"(g.inSize), "+s"(g.outSize), "+s"(g.tauMax), "+s"(g.eLen), "+s"(g.orderPitch), "+s"(g.tau0));
    asm volatile("" : "+s"(c.inCounter), "+s"(c.outCounter), "+s"(c.currCounter), "+s"(c.pStart), "+s"(c.nChunk0), "+s"(c.nSteps), "+s"(c.inMono), "+s"(c.yinCert));
    asm volatile("" : "+s"(d.voiceRing), "+s"(d.synthRing), "+s"(d.outAcc), "+s"(d.pitch), "+s"(d.eFrame), "+s"(d.outEFrame), "+s"(d.yFrame), "+s"(d.hImp));
    asm volatile("" : "+s"(d.pitchStWin), "+s"(d.hannTab), "+s"(d.hannOff), "+s"(d.notes), "+s"(d.notesN), "+s"(d.fftTw1), "+s"(d.fftTw2), "+s"(d.fftTws), "+s"(d.dbg), "+s"(d.ub), "+s"(d.gate));
}
// a workgroup barrier that orders LDS traffic only: __syncthreads() is a workgroup-scope fence + s_barrier, and the fence waits for every
// global store in flight -- the finished block's output samples, the ring write -- whose acknowledgements nobody here needs
__device__ __forceinline__ void ws_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void ws_mb_launder_carve(WsCarve &cv)
{
    asm volatile("" : "+s"(cv.xs), "+s"(cv.eF), "+s"(cv.fr), "+s"(cv.qtab), "+s"(cv.htab), "+s"(cv.P), "+s"(cv.dY), "+s"(cv.gtab), "+s"(cv.r), "+s"(cv.aPrev));
    asm volatile("" : "+s"(cv.hp), "+s"(cv.aF), "+s"(cv.xp), "+s"(cv.hist), "+s"(cv.tw), "+s"(cv.oA), "+s"(cv.st), "+s"(cv.ctl));
}
// Block `blk` of the launch is complete (the caller's barrier); on return block blk + 1 may start: c / scp / inb / outb / gateOpen are
// the next block's.  All 768 threads.  Conditions (process_ws_blocks, vp_capi.hip): pitch corrector alone with the fused prologue,
// VP_IIR_FAST, host blocks of whole chunks on the chunk grid (pStart = 0 for every block), N <= 2 x 768, C <= 768,
// span - N <= 3 x 768, latency <= F + (nSteps - 1) C.
__device__ __forceinline__ void ws_mb_boundary(VpGeom &g, VpCall &c, VpDev &d, const VpWsMb *mbp, int blk, const VpWsSched *&scp, lds_f64 *sm, WsCarve &cv,
                                               lds_ctl *ctl, lds_state *st, lds_state *stBG, lds_f64 *xsAll, lds_f64 *oE0, lds_f64 *yF0, lds_f64 *oA, double *gateRed,
                                               const float *&inb, float *&outb, int span, double &gateT, int &gateOpen)
{
    const int s = vp_stream(d), nt = blockDim.x, tid = vp_tid();
    const int N = g.N, C = g.C, mono = c.inMono, Cin = mono ? 1 : 3;
    const VpWsSched &scb = *scp;
    const int pl = scb.instPar[scb.nInst - 1];                                // where the frame in flight sits
    int nChunkEnd = c.nChunk0;
    for (int t = 0; t < c.nSteps; t++) { if (nChunkEnd == g.cpf - 1) nChunkEnd = 0; nChunkEnd += 1; }
    const int done = nChunkEnd * C;
    const int inCn = mbp->inCtr[blk + 1], outCn = mbp->outCtr[blk + 1], curCn = mbp->currCtr[blk + 1];
    const float *xb = inb + (size_t)s * Cin * N;                              // this block's slab: its last samples top the voice window up
    const float *inn = inb + (size_t)g.S * Cin * N;
    const float *xn = inn + (size_t)s * Cin * N;                              // the next block's
    float *ob = outb + (size_t)s * 2 * N;
    float *vrw = d.voiceRing + (size_t)s * g.inSize;
    // ---- requests: the next block's samples (ring write, gate, voice window), the top-up of the window from this block's slab
    float nv0[2], nv1[2] = {0.f, 0.f}, nv2[2] = {0.f, 0.f}, mv[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int k = tid + u * nt;
        nv0[u] = (k < N) ? xn[k] : 0.0f;
        if (mono == 0) { nv1[u] = (k < N) ? xn[N + k] : 0.0f; nv2[u] = (k < N) ? xn[2 * N + k] : 0.0f; }
        // window entry j = span - N + k <-> logical index L = j - toKeep of the NEXT block's ring (its own samples sit at [latency, latency + N))
        const int L = span - N + k - g.toKeep;
        mv[u] = (k < N) ? ((L < g.latency) ? xb[L - (g.latency - N)] : xn[L - g.latency]) : 0.0f;
    }
    // (the block after the next one: its slab's cache lines are requested now -- one float per 128-byte line, consumed by nothing -- so
    // that the next boundary's loads find them in L2 instead of paying the trip to HBM on the launch's critical path)
    float touch = 0.0f;
    if (blk + 2 < mbp->nBlocks) {
        const float *x2 = inn + (size_t)g.S * Cin * N + (size_t)s * Cin * N;
        const int line = tid * 32;
        if (line < Cin * N) touch = x2[line];
    }
    // ---- emit of this block (ws_emit_block without the accumulator ring: the slice lives in LDS for the whole launch)
    {
        const float *vr = d.voiceRing + (size_t)s * g.inSize;
        const float *sr0 = d.synthRing + (size_t)s * 2 * g.inSize, *sr1 = sr0 + g.inSize;
        const int dryOn = st->sp.dryOn, synthOn = st->sp.synthOn;
        const double gainVoice = st->sp.gainVoice, gainSynth = st->sp.gainSynth;
        for (int i = tid; i < N; i += nt) {
            int pin = c.currCounter + i;
            pin -= (pin >= g.inSize) ? g.inSize : 0;
            double v = oA[i];
            if (dryOn) v += (double)vr[pin] * gainVoice;
            double l = v, r = v;
            if (synthOn) { l += (double)sr0[pin] * gainSynth; r += (double)sr1[pin] * gainSynth; }
            ob[i] = (float)l;
            ob[N + i] = (float)r;
        }
    }
    // ---- what moves inside LDS: into registers first
    const double ov = (tid < C) ? oA[N + min(tid, C - 1)] : 0.0;              // the accumulator slice's overhang
    double xsv[3], so = 0.0;
#pragma unroll
    for (int u = 0; u < 3; u++) { const int j = tid + u * nt; xsv[u] = (j + N < span) ? xsAll[j + N] : 0.0; }
#pragma unroll
    for (int u = 0; u < 2; u++) { const int j = tid + u * nt; if (j < N) { const double a = xsAll[j]; so += a * a; } }   // the N samples that leave the ring
    ws_lds_barrier();
    // ---- LDS writes
    if (tid < C) oA[tid] = ov;
    for (int q = C + tid; q < N + C; q += nt) oA[q] = 0.0;
#pragma unroll
    for (int u = 0; u < 3; u++) { const int j = tid + u * nt; if (j + N < span) xsAll[j] = xsv[u]; }
    double sn = 0.0;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int k = tid + u * nt;
        if (k < N) {
            xsAll[span - N + k] = (double)mv[u];
            const double a = (double)nv0[u];
            sn += a * a;
            int p = inCn + k;
            p -= (p >= g.inSize) ? g.inSize : 0;
            vrw[p] = nv0[u];                                                  // MyBuffer::fillInputBuffers (MyBuffer.cpp:74-105)
            if (mono != 2) {
                float *sr0 = d.synthRing + (size_t)s * 2 * g.inSize;
                sr0[p] = nv1[u];
                sr0[g.inSize + p] = nv2[u];
            }
        }
    }
    for (int i = tid; i < (int)(sizeof(WsCtl) / sizeof(int)); i += nt) ((lds_i32 *)ctl)[i] = 0;
    {   // the background's private copy of the tracker state starts from the group's again
        const lds_i32 *src = (const lds_i32 *)st;
        lds_i32 *dst = (lds_i32 *)stBG;
        for (int i = tid; i < (int)(sizeof(VpPitchState) / sizeof(int)); i += nt) dst[i] = src[i];
    }
    if (pl == 1 && nChunkEnd != 0 && st->nAn != 0) {
        // the frame in flight ended in the parity-1 buffers: a block's schedule expects it in parity 0 (what the prologue of a launch of
        // its own would have loaded there from HBM: the same ranges)
        const lds_f64 *oE1 = oE0 + 3 * g.F + 2048, *yF1 = oE0 + 2 * g.F + 2048;
        for (int i = done + tid; i < g.F; i += nt) oE0[i] = oE1[i];
        for (int i = max(0, done - g.orderPitch) + tid; i < done; i += nt) yF0[i] = yF1[i];
        if (tid < WS_HP(g)) (sm + cv.hp)[tid] = (sm + cv.hp + WS_HP(g))[tid];
        if (tid < WS_AF(g)) (sm + cv.aF)[tid] = (sm + cv.aF + WS_AF(g))[tid];
    }
    {
        const double part = wave_sum(sn - so);
        if ((tid & 63) == 0) gateRed[tid >> 6] = part;
    }
    ws_lds_barrier();
    // ---- the gate of the next block (see the prologue): the ring's sum of squares updated, decided outside the rounding band -- which
    // widens with every incremental update --, else by the reference's sequential sum over the ring (which then also resets the drift).
    // The bound: every rounding since the last exact sum (the prologue's tree sum or a fallback's sequential one) is at most u times an
    // operand, and every operand is a partial sum of squares of the ring (<= T), of the new samples or of the leaving ones; both of the
    // latter are <= T_before + T_after.  So with M = the largest T since that exact sum, the drift is <= 2 M u (2 N + 64) per update,
    // on top of the exact sum's own (2 inSize + 64) M u against the reference's order.  M, not the current T: after a loud passage has
    // left the ring T is orders of magnitude smaller than the rounding its sums left behind.  M lives in gateRed[16] (in LDS: a register
    // more spilled around the block loop); thread 0 raises it while the others may still read it -- fmax with the raised value gives
    // the same Tm.
    {
        double T = gateT;
#pragma unroll
        for (int w = 0; w < 16; w++) T += gateRed[w];
        const double Tm = fmax(gateRed[16], T);
        const double band = Tm * vp_f64_here(2 * g.inSize + 64 + 2 * (blk + 1) * (2 * N + 64)) * 1.1102230246251565e-16 * 1.5;
        gateT = T;
        if (tid == 0) gateRed[16] = Tm;
        if (T - g.gateThrSum > band) gateOpen = 1;
        else if (g.gateThrSum - T > band) gateOpen = 0;
        else {
            __threadfence_block();                                            // (the ring write above: complete before thread 0 reads the ring)
            __syncthreads();
            if (tid == 0) {
                const float *vr = d.voiceRing + (size_t)s * g.inSize;
                double seq = 0.0;                                             // AudioBuffer::getRMSLevel order
                for (int i = 0; i < g.inSize; i++) { double a = (double)vr[i]; seq += a * a; }
                ctl->ishareP[0] = !(seq < g.gateThrSum);
                gateRed[15] = seq;
            }
            __syncthreads();
            gateOpen = ctl->ishareP[0];
            gateT = gateRed[15];
            __syncthreads();
            if (tid == 0) { ctl->ishareP[0] = 0; gateRed[15] = 0.0; gateRed[16] = gateT; }   // (an exact sum again: the drift starts from it)
        }
        if (tid == 0) d.gate[s * 2 + 0] = gateOpen;
    }
    asm volatile("" :: "v"(touch));
    // ---- the next block's arguments
    c.inCounter = inCn; c.outCounter = outCn; c.currCounter = curCn; c.nChunk0 = mbp->nChunk0[blk + 1];
    scp = &mbp->sc[mbp->schedOf[blk + 1]];
    inb = inn;
    outb += (size_t)g.S * 2 * N;
    ws_mb_launder(g, c, d);
    ws_mb_launder_carve(cv);
}

#define WS_IS_LEAN false
#include "vp_pitch_ws_body.inc"
#define WS_MB 1
#include "vp_pitch_ws_body.inc"
#undef WS_MB
#undef WS_IS_LEAN
#if VP_TU_HAS(6)
__global__ __launch_bounds__(768) void vp_k_pitch_ws(VpGeom g, VpCall c, VpDev d, VpWsSched sc, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body<true, false>(g, c, d, sc, in, out, smem);
}
__global__ __launch_bounds__(768) void vp_k_pitch_ws_x(VpGeom g, VpCall c, VpDev d, VpWsSched sc, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body<false, false>(g, c, d, sc, in, out, smem);
}
#endif
#if VP_TU_HAS(6)
// several queued blocks per launch (vp_process_blocks*_device, pitch corrector alone): see pitch_ws_body
__global__ __launch_bounds__(768) void vp_k_pitch_ws_mb(VpGeom g, VpCall c, VpDev d, VpWsMb mb, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body_mb<true, false>(g, c, d, &mb, in, out, smem);
}
#endif
#if VP_TU_HAS(7)
// lpcPitch 16 .. WS_ORDER_MAX (round 6)
__global__ __launch_bounds__(768) void vp_k_pitch_ws_o24(VpGeom g, VpCall c, VpDev d, VpWsSched sc, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body<true, true>(g, c, d, sc, in, out, smem);
}
__global__ __launch_bounds__(768) void vp_k_pitch_ws_x_o24(VpGeom g, VpCall c, VpDev d, VpWsSched sc, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body<false, true>(g, c, d, sc, in, out, smem);
}
#endif
#if VP_TU_HAS(8)
// ... in the exact arithmetic, and for lpcPitch 16 .. WS_ORDER_MAX (the block boundary is the same: the exact recursion keeps no state of
// its own between chunks -- its history is read back from the frame's outputs -- and every windowed add of a block is flushed before
// the block's last barrier)
__global__ __launch_bounds__(768) void vp_k_pitch_ws_x_mb(VpGeom g, VpCall c, VpDev d, VpWsMb mb, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body_mb<false, false>(g, c, d, &mb, in, out, smem);
}
#endif
#if VP_TU_HAS(9)
__global__ __launch_bounds__(768) void vp_k_pitch_ws_mb_o24(VpGeom g, VpCall c, VpDev d, VpWsMb mb, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body_mb<true, true>(g, c, d, &mb, in, out, smem);
}
__global__ __launch_bounds__(768) void vp_k_pitch_ws_x_mb_o24(VpGeom g, VpCall c, VpDev d, VpWsMb mb, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body_mb<false, true>(g, c, d, &mb, in, out, smem);
}
#endif
#if VP_TU_HAS(10)
#define WS_IS_LEAN true
#define WS_LEAN 1
#include "vp_pitch_ws_body.inc"
#undef WS_LEAN
#undef WS_IS_LEAN
// The lean build of vp_k_pitch_ws (FAST, one block per launch) for the launch shape of the plugin's own geometry at 44.1 kHz:
// see pitch_ws_body_l.  Selected by the host alone (vp_capi.hip pitch_ws_lean_ok); everything else keeps the generic builds.
__global__ __launch_bounds__(768) void vp_k_pitch_ws_l(VpGeom g, VpCall c, VpDev d, VpWsSched sc, const float *__restrict__ in, float *__restrict__ out)
{
    extern __shared__ double smem[];
    pitch_ws_body_l(g, c, d, sc, in, out, smem);
}
#endif
