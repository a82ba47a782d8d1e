// demod_audio_tile.inc -- one workgroup's tile of 256 audio samples (gain, volume, audio FIRs):
// the body of demod_audio_kernel and of demod_bank_audio_kernel (demod.hip).
// Expects `a` (a DemodLaunch) and DEMOD_TILE (the tile index) in scope.
    __shared__ float vb[kVMax], yb[kY1Max], t1[kMaxAudioTaps], t2[kMaxAudioTaps];
    const int tid = threadIdx.x;
    const long long o0 = (long long)(DEMOD_TILE) * kTile;
    const int nloc = (int)min((long long)kTile, a.n_audio - o0);
    if (a.sink == 0) {
        if (tid < nloc) a.out[o0 + tid] = v_at(a, o0 + tid);
        return;
    }
    if (tid < a.T1) t1[tid] = a.taps[TP_A1 + tid];
    if (tid < a.T2) t2[tid] = a.taps[TP_A2 + tid];
    if (a.sink == 1) {
        const long long clo = c1_of(a, o0) - (a.T1 - 1), chi = c1_of(a, o0 + nloc - 1);
        const int nv = (int)(chi - clo + 1);
        for (int i = tid; i < nv; i += kTile) vb[i] = v_at(a, clo + i);
        __syncthreads();
        if (tid < nloc) {
            const float *x = vb + (int)(c1_of(a, o0 + tid) - clo);
            float s = 0.0f;
            for (int k = 0; k < a.T1; k++) s = s + t1[k] * x[-k];
            a.out[o0 + tid] = s;
        }
        return;
    }
    // audioFilter2 output o has its newest input at audioFilter1 output r(o) of this call
    const long long r_first = (a.a2_out0 + o0) * kA2Dec + (kA2Dec - 1) - a.a2_in0;
    const long long rlo = r_first - (a.T2 - 1), rhi = r_first + (long long)(nloc - 1) * kA2Dec;
    const long long rclo = rlo < 0 ? 0 : rlo;
    const int nhist = (int)(rclo - rlo), nr = (int)(rhi - rlo + 1);
    const long long vlo = c1_of(a, rclo) - (a.T1 - 1), vhi = c1_of(a, rhi);
    const int nv = (int)(vhi - vlo + 1);
    for (int i = tid; i < nv; i += kTile) vb[i] = v_at(a, vlo + i);
    for (int j = tid; j < nhist; j += kTile) yb[j] = a.st[ST_A2 + a.T2 - 1 + rlo + j];
    __syncthreads();
    for (int j = nhist + tid; j < nr; j += kTile) {
        const float *x = vb + (int)(c1_of(a, rlo + j) - vlo);
        float s = 0.0f;
        for (int k = 0; k < a.T1; k++) s = s + t1[k] * x[-k];
        yb[j] = s;
    }
    __syncthreads();
    if (tid < nloc) {
        const float *y = yb + (a.T2 - 1) + tid * kA2Dec;
        float s = 0.0f;
        for (int k = 0; k < a.T2; k++) s = s + t2[k] * y[-k];
        a.out[o0 + tid] = s;
    }
