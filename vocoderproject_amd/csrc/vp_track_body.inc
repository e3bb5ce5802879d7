// vp_track_body.inc -- the decision of one wavefront from its staged window, included by vp_k_yin_track and vp_k_yin_track_stream
// (csrc/vp_track.hip): the sums, the normalisation carry, the ballot walk and the note lookup.  The text is the same for both kernels, so
// their decisions are the same statements.  In scope: xs (the wavefront's slice, staged), lane, F, tauMax, nf0, nf1, notesN, A.fs, A.tau0.
// Leaves: tau (uniform) and ratio.
    // d[8 lane + j] = sum over i of (x[i] - x[i + 8 lane + j])^2, i ascending; w[m] = x[i0 + 8 lane + m]
    double acc[VP_TRACK_LAGS], w[2 * VP_TRACK_LAGS];
    const trk_lds_f32 *wl = xs + TRK_ROW * lane;
#pragma unroll
    for (int j = 0; j < VP_TRACK_LAGS; j++) { acc[j] = 0.0; w[j] = (double)wl[j]; }
    for (int blk = 0; blk < F / 8; blk++) {
        const trk_lds_f32 *nx = wl + TRK_ROW * (blk + 1), *vb = xs + TRK_ROW * blk;
        double v[8];
#pragma unroll
        for (int m = 0; m < 8; m++) { w[8 + m] = (double)nx[m]; v[m] = (double)vb[m]; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
#pragma unroll
            for (int j = 0; j < VP_TRACK_LAGS; j++) {
                const double d = v[u] - w[u + j];
                acc[j] += d * d;
            }
        }
#pragma unroll
        for (int m = 0; m < 8; m++) w[m] = w[8 + m];
    }
    trk_wave_sync();                                                          // (the slice is rewritten below)

    // :395-403: d[0] = 1, tmp += d[k], d[k] *= k / tmp in increasing k -- tmp starts at 0 and 0 + d[1] is d[1], so lag 0 enters as 0
    if (lane == 0) acc[0] = 0.0;
    double cum[VP_TRACK_LAGS], carry = 0.0;
#pragma unroll
    for (int j = 0; j < VP_TRACK_LAGS; j++) cum[j] = 1.0;
    const int nOwners = (tauMax + VP_TRACK_LAGS - 1) / VP_TRACK_LAGS;
    for (int l = 0; l < nOwners; l++) {
        double t = carry;
        if (lane == l) {
#pragma unroll
            for (int j = 0; j < VP_TRACK_LAGS; j++) { t += acc[j]; cum[j] = t; }
        }
        carry = trk_readlane(t, l);
    }
    trk_lds_f64 *dn = (trk_lds_f64 *)xs;
#pragma unroll
    for (int j = 0; j < VP_TRACK_LAGS; j++) {
        const int k = VP_TRACK_LAGS * lane + j;
        const double q = (double)k / cum[j];
        double y = acc[j] * q;                                                // (silence: 0 * inf = NaN, which fails the tolerance test)
        if (k == 0) y = 1.0;
        if (k >= tauMax) y = 0.0;                                             // the guard slot d[tauMax] = 0; lags behind it are not read
        dn[k] = y;
    }
    if (lane == 0) dn[TRK_MAXLAG] = 0.0;                                      // (the guard slot at tauMax = 512)
    trk_wave_sync();

    // :429-447 on ballots, lag 64 q + lane: under[q] = d[k] < yinTol for tau0 <= k < tauMax, stop[q] = !(d[k + 1] < d[k])
    unsigned long long under[TRK_MAXLAG / 64], stop[TRK_MAXLAG / 64];
#pragma unroll
    for (int q = 0; q < TRK_MAXLAG / 64; q++) {
        const int k = 64 * q + lane;
        const double y0 = dn[k], y1 = dn[k + 1];
        under[q] = __ballot(k >= A.tau0 && k < tauMax && y0 < 0.25);
        stop[q] = __ballot(!(y1 < y0));
    }
    int first = INT_MAX;                                                      // first lag under the tolerance
#pragma unroll
    for (int q = TRK_MAXLAG / 64 - 1; q >= 0; q--)
        if (under[q]) first = 64 * q + (int)__builtin_ctzll(under[q]);
    int tau = 0;
    if (first != INT_MAX) {
        int ks = TRK_MAXLAG;                                                  // first lag >= first at which the descent stops
#pragma unroll
        for (int q = TRK_MAXLAG / 64 - 1; q >= 0; q--) {
            unsigned long long m = stop[q];
            if (64 * q + 63 < first) m = 0;
            else if (64 * q < first) m &= ~0ULL << (first - 64 * q);
            if (m) ks = 64 * q + (int)__builtin_ctzll(m);
        }
        // the walk leaves at tauMax - 1 without looking further (:438-439); started there, it looks once, at the guard slot
        if (first + 1 >= tauMax) tau = ks > first ? first + 1 : first;
        else tau = ks < tauMax - 1 ? ks : tauMax - 1;
    }
    tau = __builtin_amdgcn_readfirstlane(tau);

    double ratio = 1.0;
    if (tau > 0) {
        // Notes::getClosestFreq (Notes.cpp:79-110): lower_bound = entries below the pitch; idx == size reads the popped slot (:99)
        const double pitch = A.fs / tau;
        const int idx = __builtin_amdgcn_readfirstlane(__popcll(__ballot(lane < notesN && nf0 < pitch)) + __popcll(__ballot(lane + 64 < notesN && nf1 < pitch)));
        const double fi = idx >= 64 ? trk_readlane(nf1, idx & 63) : trk_readlane(nf0, idx & 63);
        double closest = fi;
        if (idx > 0) {
            const int im = idx - 1;
            const double fim = im >= 64 ? trk_readlane(nf1, im & 63) : trk_readlane(nf0, im & 63);
            if (!(fabs(fi - pitch) <= fabs(fim - pitch))) closest = fim;
        }
        ratio = closest / pitch;                                              // :595-596
    }
