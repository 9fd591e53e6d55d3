/* C restatement of the IQ corrector's arithmetic contract (include/fmdemod.h, "DC offset and IQ imbalance correction"): the conversion,
 * the moments in their fixed summation order, the solve step and the fp32 apply step.  Built by tests/iqcorr_ref.py with
 * gcc -O2 -ffp-contract=off -fno-fast-math, so every operation is the one written. */
#include <math.h>
#include <stdint.h>

#define CHUNK 4096
#define LANES 256

/* fmt 0: cf32 as is; 1: u8, v - 127; 2: s8; 3: s16.  raw and out hold n pairs. */
void iqcorr_ref_convert(const void* raw, int fmt, long long n, float* out) {
    for (long long k = 0; k < 2 * n; k++) {
        switch (fmt) {
            case 0: out[k] = ((const float*)raw)[k]; break;
            case 1: out[k] = (float)((const uint8_t*)raw)[k] - 127.0f; break;
            case 2: out[k] = (float)((const int8_t*)raw)[k]; break;
            default: out[k] = (float)((const int16_t*)raw)[k]; break;
        }
    }
}

static double tree(double* p) {
    for (int h = LANES / 2; h >= 1; h /= 2)
        for (int j = 0; j < h; j++) p[j] += p[j + h];
    return p[0];
}

/* x: n converted pairs, the samples 0 .. n - 1 since reset.  out: n, sum i, sum q, sum i^2, sum q^2, sum i q. */
void iqcorr_ref_moments(const float* x, long long n, double* out) {
    double total[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long c0 = 0; c0 < n; c0 += CHUNK) {
        double p[5][LANES];
        for (int m = 0; m < 5; m++)
            for (int j = 0; j < LANES; j++) p[m][j] = 0.0;
        const long long c1 = c0 + CHUNK < n ? c0 + CHUNK : n;
        for (long long s = c0; s < c1; s++) {          /* ascending s: every lane j = s mod 256 sees its k = (s - c0) / 256 ascending */
            const int j = (int)((s - c0) % LANES);
            const double di = (double)x[2 * s], dq = (double)x[2 * s + 1];
            p[0][j] += di;
            p[1][j] += dq;
            p[2][j] += di * di;
            p[3][j] += dq * dq;
            p[4][j] += di * dq;
        }
        /* a complete chunk joins the total; an open last chunk is reported as total + tree, which is the same addition */
        for (int m = 0; m < 5; m++) total[m] += tree(p[m]);
    }
    out[0] = (double)n;
    for (int m = 0; m < 5; m++) out[1 + m] = total[m];
}

/* m: the six moments; out: dc_i, dc_q, w_re, w_im.  Returns 0, or -1 where the library returns FMD_ERR_ARG. */
int iqcorr_ref_solve(const double* m, float* out) {
    for (int k = 0; k < 6; k++)
        if (!isfinite(m[k])) return -1;
    const double n = m[0];
    if (!(n > 0.0)) return -1;
    const double mi = m[1] / n, mq = m[2] / n;
    const double vii = m[3] / n - mi * mi;
    const double vqq = m[4] / n - mq * mq;
    const double viq = m[5] / n - mi * mq;
    const double p = vii + vqq;
    const double cr = vii - vqq, ci = 2.0 * viq;
    const double d = p * p - (cr * cr + ci * ci);
    const double s = sqrt(d > 0.0 ? d : 0.0);
    double wr = 0.0, wi = 0.0;
    if (p + s > 0.0) {
        wr = -cr / (p + s);
        wi = -ci / (p + s);
    }
    const float r[4] = {(float)mi, (float)mq, (float)wr, (float)wi};
    for (int k = 0; k < 4; k++)
        if (!isfinite(r[k])) return -1;
    for (int k = 0; k < 4; k++) out[k] = r[k];
    return 0;
}

/* y = z + w conj(z), z = x - dc, in fp32 */
void iqcorr_ref_apply(const float* x, long long n, const float* corr, float* y) {
    const float dc_i = corr[0], dc_q = corr[1], w_re = corr[2], w_im = corr[3];
    for (long long s = 0; s < n; s++) {
        const float zi = x[2 * s] - dc_i, zq = x[2 * s + 1] - dc_q;
        y[2 * s] = fmaf(w_re, zi, fmaf(w_im, zq, zi));
        y[2 * s + 1] = fmaf(w_im, zi, fmaf(-w_re, zq, zq));
    }
}
