// demod_stage1_tile.inc -- one workgroup's tile of 256 pre-gain values: the body of
// demod_stage1_kernel and of demod_bank_stage1_kernel (demod.hip), included as text so
// that both compile exactly the same statements in the same order.
// Expects `a` (a DemodLaunch) and DEMOD_TILE (the tile index) in scope.
    __shared__ float xr[kInMax], xi[kInMax], fr[kFlMax], fi[kFlMax];
    __shared__ float tu[kMaxUserTaps], tbr[kMaxBandTaps], tbi[kMaxBandTaps];
    const int tid = threadIdx.x;
    const long long m0 = (long long)(DEMOD_TILE) * kTile;
    const int nloc = (int)min((long long)kTile, a.npre - m0);
    if (tid < a.Tu) tu[tid] = a.taps[TP_UF + tid];
    if (a.kind == kKindBand && tid < a.Tb) {
        tbr[tid] = a.taps[TP_BPR + tid];
        tbi[tid] = a.taps[TP_BPI + tid];
    }
    const long long f_first = fidx(a, m0), f_last = fidx(a, m0 + nloc - 1);
    const int halo = a.kind == kKindBand ? a.Tb - 1 : (a.kind == kKindFm ? 1 : 0);
    const long long flo = f_first - halo, fclo = flo < 0 ? 0 : flo;
    const int nhist = (int)(fclo - flo);                 // samples older than this call
    const int ncomp = (int)(f_last - fclo + 1);          // user-filtered samples to compute
    const int nin = ncomp + a.Tu - 1;
    const long long ilo = fclo + a.skip - (a.Tu - 1);
    for (int i = tid; i < nin; i += kTile) {
        float r, s;
        in_at(a, ilo + i, r, s);
        xr[i] = r;
        xi[i] = s;
    }
    for (int j = tid; j < nhist; j += kTile) {
        const long long f = flo + j;                      // < 0
        if (a.kind == kKindBand) {
            fr[j] = a.st[ST_BP_RE + a.Tb - 1 + f];
            fi[j] = a.st[ST_BP_IM + a.Tb - 1 + f];
        } else {                                          // FM: carryOverSamples
            fr[j] = a.st[ST_CARRY];
            fi[j] = a.st[ST_CARRY + 1];
        }
    }
    __syncthreads();
    for (int j = tid; j < ncomp; j += kTile) {
        float sr = 0.0f, si = 0.0f;
        const float *pr = xr + j + a.Tu - 1, *pi = xi + j + a.Tu - 1;
        for (int k = 0; k < a.Tu; k++) {
            sr = sr + tu[k] * pr[-k];
            si = si + tu[k] * pi[-k];
        }
        fr[nhist + j] = sr;
        fi[nhist + j] = si;
    }
    __syncthreads();
    if (tid >= nloc) return;
    const long long m = m0 + tid;
    const int j = (int)(fidx(a, m) - flo);
    float v;
    if (a.kind == kKindAm) {
        v = fr[j] * fr[j] + fi[j] * fi[j];
    } else if (a.kind == kKindFm) {
        const float cr = fr[j] * fr[j - 1] + fi[j] * fi[j - 1];
        const float ci = fi[j] * fr[j - 1] - fr[j] * fi[j - 1];
        v = a.qgain * (float)atan2((double)ci, (double)cr);
    } else {
        float s = 0.0f;                                   // only the real part is ever used
        for (int k = 0; k < a.Tb; k++) s = s + (tbr[k] * fr[j - k] - tbi[k] * fi[j - k]);
        v = s;
    }
    a.pre[m] = v;
