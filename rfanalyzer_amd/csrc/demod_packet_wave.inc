// demod_packet_wave.inc -- one wave takes a packet's maximum and, for AM, its sum in index
// order: the body of demod_packet_kernel and of demod_bank_packet_kernel (demod.hip).
// Expects `a` (a DemodLaunch) and DEMOD_TILE (the packet index) in scope.
    __shared__ float buf[64];
    const long long p = DEMOD_TILE;
    const int lane = threadIdx.x;
    const long long X0 = p * a.ps, X1 = min((p + 1) * a.ps, a.n);
    const long long lo = pre_lower(a, X0), hi = pre_lower(a, X1);
    float m = -INFINITY;
    for (long long q = lo + lane; q < hi; q += 64) {
        const float x = a.pre[q];
        if (x > m) m = x;                                 // NaN never wins, as in the reference
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(m, off);
        if (o > m) m = o;
    }
    float avg = 0.0f;
    if (a.kind == kKindAm) {
        float s = 0.0f;
        for (long long base = lo; base < hi; base += 64) {
            buf[lane] = base + lane < hi ? a.pre[base + lane] : 0.0f;
            __syncthreads();
            if (lane == 0) {
                const int cnt = (int)min(64LL, hi - base);
                for (int j = 0; j < cnt; j++) s = s + buf[j];
            }
            __syncthreads();
        }
        avg = s / (float)(int)(hi - lo);
    }
    if (lane == 0) {
        a.pk_max[p] = m;
        a.pk_avg[p] = avg;
    }
