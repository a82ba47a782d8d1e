// ddc_fir_tile.inc -- one workgroup's tile of P decimated outputs: the body of
// ddc_fir_kernel and of ddc_bank_kernel (ddc.hip), included as text so that the
// single-handle kernel is compiled from exactly the statements it always had.
// Expects `a` (a DdcLaunch, by value) and DDC_TILE (the tile index) in scope.
    extern __shared__ __attribute__((aligned(16))) v2f dyn[];
    // [taps of the chunk | mixer table (cos, sin), L entries | staged samples]
    float *wl = reinterpret_cast<float *>(dyn);
    float2 *cs = reinterpret_cast<float2 *>(dyn + a.kc_pad / 2);
    v2f *xs = dyn + a.kc_pad / 2 + a.cs_v2;
    const int tid = threadIdx.x;
    const int nth = blockDim.x;
    for (int i = tid; i < a.L; i += nth) cs[i] = float2{a.cosv[i], a.sinv[i]};
    __syncthreads();
    const int D = a.D, Dp = a.D + a.pad;                   // LDS layout: rows of D samples
    const long long m0 = (long long)(DDC_TILE) * a.P;
    const int nloc = (int)min((long long)a.P, a.n_out - m0);
    const bool valid = tid < nloc;
    // newest input of output n (global indices), RationalResampler / FirFilter counters closed-form
    const long long nf = a.n0 + m0, nl = nf + (nloc - 1), nt = nf + (valid ? tid : 0);
    const long long cf = (nf * a.Dd + a.off) / a.I, cl = (nl * a.Dd + a.off) / a.I;
    const long long pos_t = nt * a.Dd + a.off;
    const int lane_off = (int)(pos_t / a.I - cf);          // decimator: tid * D
    const int phase = (int)(pos_t % a.I);
    const long long jb = cf - a.in0;                        // call-relative input index of output m0
    const int step = a.L > 0 ? nth % a.L : 0;
    const int srow = nth / D, scol = nth % D;
    v2f acc = {0.0f, 0.0f};
    for (int k0 = 0; k0 < a.T; k0 += a.KC) {
        const int k1 = min(a.T, k0 + a.KC);
        const long long lo = jb - (k1 - 1);                 // oldest sample any lane needs
        const int span = (int)(cl - cf) + (k1 - k0);         // fits the LDS the host sized
        if (a.I == 1)
            for (int i = tid; i < k1 - k0; i += nth) wl[i] = a.taps[k0 + i];
        // leading samples older than this call come from the history (first workgroups only)
        const int nh = (int)min((long long)span, max(0LL, -lo));
        for (int i = tid; i < nh; i += nth) {
            float re, im;
            ddc_sample<FMT>(a, lo + i, 0, re, im);
            xs[(i / D) * Dp + i % D] = v2f{re, im};
        }
        // raw part: U loads in flight per lane before any is converted
        constexpr int U = 8;
        bool staged = false;
        if constexpr (FMT != RFA_IN_F32_INTERLEAVED) {
            if (a.vec4) {
                // 4 consecutive samples per load (8 B for 8-bit IQ, 16 B for int16): four
                // times the bytes in flight of the per-sample loop, which left HBM latency
                // exposed.  Groups are aligned in the raw buffer; samples outside
                // [lo + nh, lo + span) are skipped.
                using R4 = typename Raw4Of<FMT>::type;
                const long long gA = lo + nh, gB = lo + span;     // gA >= 0 whenever gA < gB
                const long long q0 = gA >> 2;
                // whole groups inside the buffer only; the last < 4 samples of the call
                // (a group that would run past raw[S-1]) go through scalar loads below
                const long long qend = min((gB + 3) >> 2, a.S >> 2);
                const int nq = gA < gB ? (int)max(0LL, qend - q0) : 0;
                const int step4 = (4 * nth) % max(a.L, 1);
                const int srow4 = (4 * nth) / D, scol4 = (4 * nth) % D;
                const int i0 = (int)((q0 + tid) * 4 - lo);          // may be negative for the first group
                int tq = cos_index(a, lo + i0);
                int rq = (i0 >= 0 ? i0 / D : -((-i0 + D - 1) / D)), cq = i0 - rq * D;
                for (int qb = tid; qb < nq; qb += U * nth) {
                    R4 v[U];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const int q = qb + u * nth;
                        if (q < nq) v[u] = static_cast<const R4 *>(a.raw)[q0 + q];
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const int q = qb + u * nth;
                        if (q < nq) {
                            const int ib = (int)((q0 + q) * 4 - lo);
                            // the group's four table entries are read before any is used, so
                            // one LDS round trip covers the group instead of four
                            float2 cst[4];
                            int t = tq;
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                cst[e] = cs[t];
                                if (++t >= a.L) t = 0;
                            }
                            int r = rq, c = cq;
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                const int i = ib + e;
                                if (i >= nh && i < span) {
                                    float re, im;
                                    mix_raw<FMT>(raw4_elem<FMT>(v[u], e), cst[e].x, cst[e].y, re, im);
                                    xs[r * Dp + c] = v2f{re, im};
                                }
                                if (++c >= D) c = 0, r++;
                            }
                        }
                        tq += step4;
                        if (tq >= a.L) tq -= a.L;
                        rq += srow4;
                        cq += scol4;
                        if (cq >= D) cq -= D, rq++;
                    }
                }
                const long long gt = max(gA, (a.S >> 2) << 2);     // scalar tail [gt, gB)
                for (long long g = gt + tid; g < gB; g += nth) {
                    const int i = (int)(g - lo);
                    float re, im;
                    ddc_sample<FMT>(a, g, cos_index(a, g), re, im);
                    xs[(i / D) * Dp + i % D] = v2f{re, im};
                }
                staged = true;
            }
        }
        if (!staged) {
            const int i0 = nh + tid;
            int t = cos_index(a, lo + i0);
            int row = i0 / D, col = i0 % D;
            for (int base = i0; base < span; base += U * nth) {
                typename RawOf<FMT>::type v[U];
    #pragma unroll
                for (int u = 0; u < U; u++) {
                    const int i = base + u * nth;
                    if (i < span) v[u] = load_raw<FMT>(a, lo + i);
                }
    #pragma unroll
                for (int u = 0; u < U; u++) {
                    const int i = base + u * nth;
                    if (i < span) {
                        float re, im;
                        const float2 cst = FMT == RFA_IN_F32_INTERLEAVED ? float2{0.0f, 0.0f} : cs[t];
                        mix_raw<FMT>(v[u], cst.x, cst.y, re, im);
                        xs[row * Dp + col] = v2f{re, im};
                    }
                    t += step;
                    if (t >= a.L) t -= a.L;
                    row += srow;
                    col += scol;
                    if (col >= D) col -= D, row++;
                }
            }
        }
        __syncthreads();
        if (valid && a.pad) {
            // decimator, even D: tap k reads staged sample tid*D + rel, rel = k1-1-k, in row segments
            int k = k0;
            while (k < k1) {
                const int rel = k1 - 1 - k;
                const int r = rel / D, c = rel - r * D;
                const int seg = min(c + 1, k1 - k);
                const v2f *x = xs + (tid + r) * Dp + c;
                const float *w = wl + (k - k0);
#pragma unroll 8
                for (int u = 0; u < seg; u++) acc = acc + w[u] * lds_ld(x - u);
                k += seg;
            }
        } else if (valid) {
            // linear layout: one contiguous walk; taps shared (I == 1, LDS) or this lane's phase row
            const v2f *x = xs + lane_off + (k1 - 1 - k0);
            if (a.I == 1) {
#pragma unroll 8
                for (int u = 0; u < k1 - k0; u++) acc = acc + wl[u] * lds_ld(x - u);
            } else {
                const float *w = a.taps + (long long)phase * a.T + k0;
#pragma unroll 8
                for (int u = 0; u < k1 - k0; u++) acc = acc + w[u] * lds_ld(x - u);
            }
        }
        __syncthreads();
    }
    if (valid) {
        a.out_re[m0 + tid] = acc.x;
        a.out_im[m0 + tid] = acc.y;
    }
