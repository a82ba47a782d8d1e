// demod_state_block.inc -- one workgroup writes every piece of state the next call needs:
// the body of demod_state_kernel and of demod_bank_state_kernel (demod.hip).
// Expects `a` (a DemodLaunch) in scope.
    const int t = threadIdx.x;
    if (t == 0) {
        float lm = a.st[ST_LMAX];
        if (a.agc) {
            for (long long p = 0; p < a.K; p++) {
                lm = lm * 0.95f;
                const float m = a.pk_max[p];
                if (m > lm) lm = m;
                a.pk_gain[p] = 0.75f / lm;
            }
        }
        a.nst[ST_LMAX] = lm;
    }
    if (t < kMaxUserTaps) {
        float r = 0.0f, s = 0.0f;
        if (t < a.Tu - 1) in_at(a, a.n - (a.Tu - 1) + t, r, s);
        a.nst[ST_UF_RE + t] = r;
        a.nst[ST_UF_IM + t] = s;
    }
    if (t < kMaxBandTaps) {
        float r = a.st[ST_BP_RE + t], s = a.st[ST_BP_IM + t];
        if (a.kind == kKindBand && t < a.Tb - 1) {
            const long long f = a.F - (a.Tb - 1) + t;
            if (f < 0) {
                r = a.st[ST_BP_RE + a.Tb - 1 + f];
                s = a.st[ST_BP_IM + a.Tb - 1 + f];
            } else {
                filt_at(a, f, r, s);
            }
        }
        a.nst[ST_BP_RE + t] = r;
        a.nst[ST_BP_IM + t] = s;
    }
    if (t == 0) {
        float r = a.st[ST_CARRY], s = a.st[ST_CARRY + 1];
        if (a.kind == kKindFm && a.F > 0) filt_at(a, a.F - 1, r, s);
        a.nst[ST_CARRY] = r;
        a.nst[ST_CARRY + 1] = s;
    }
    __syncthreads();                                      // the gains of this call are written
    if (t < kMaxAudioTaps) {
        float v = a.st[ST_A1 + t];
        if (a.sink >= 1 && t < a.T1 - 1) v = v_at(a, a.npre - (a.T1 - 1) + t);
        a.nst[ST_A1 + t] = v;
        float y = a.st[ST_A2 + t];
        if (a.sink == 2 && t < a.T2 - 1) y = y1_at(a, a.ny1 - (a.T2 - 1) + t);
        a.nst[ST_A2 + t] = y;
    }
