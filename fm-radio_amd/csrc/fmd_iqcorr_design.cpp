// Built with -ffp-contract=off -fno-fast-math (Makefile): every double operation is the one written, so the solve step is the pure
// function of the moments that tests/cpp/iqcorr_ref.c restates.
#include "fmd_iqcorr_design.h"

#include <cmath>

namespace fmd {

std::string& iqcorr_global_error() {
    thread_local std::string e;
    return e;
}

double iqcorr_tree(double* p) {
    for (int h = kIqLanes / 2; h >= 1; h >>= 1)
        for (int j = 0; j < h; j++) p[j] += p[j + h];
    return p[0];
}

bool iqcorr_finite(const fmd_iq_correction& c) {
    return std::isfinite(c.dc_i) && std::isfinite(c.dc_q) && std::isfinite(c.w_re) && std::isfinite(c.w_im);
}

int iqcorr_solve(const fmd_iq_moments* m, fmd_iq_correction* out, std::string* err) {
    if (!m || !out) { *err = "null moments or output"; return FMD_ERR_ARG; }
    if (!(m->n > 0) || !std::isfinite(m->n)) { *err = "no samples: n must be finite and > 0"; return FMD_ERR_ARG; }
    if (!(std::isfinite(m->sum_i) && std::isfinite(m->sum_q) && std::isfinite(m->sum_ii) && std::isfinite(m->sum_qq) && std::isfinite(m->sum_iq))) {
        *err = "a moment is not finite";
        return FMD_ERR_ARG;
    }
    const double mi = m->sum_i / m->n, mq = m->sum_q / m->n;
    const double vii = m->sum_ii / m->n - mi * mi;
    const double vqq = m->sum_qq / m->n - mq * mq;
    const double viq = m->sum_iq / m->n - mi * mq;
    const double p = vii + vqq;
    const double cr = vii - vqq, ci = 2.0 * viq;
    const double d = p * p - (cr * cr + ci * ci);
    const double s = std::sqrt(d > 0.0 ? d : 0.0);
    const double den = p + s;
    double wr = 0.0, wi = 0.0;
    if (den > 0.0) { wr = -cr / den; wi = -ci / den; }
    const fmd_iq_correction c{(float)mi, (float)mq, (float)wr, (float)wi};
    if (!iqcorr_finite(c)) { *err = "the correction is not finite in fp32"; return FMD_ERR_ARG; }
    *out = c;
    return FMD_OK;
}

}  // namespace fmd

extern "C" int fmd_iqcorr_solve(const fmd_iq_moments* m, fmd_iq_correction* out) {
    return fmd::iqcorr_solve(m, out, &fmd::iqcorr_global_error());
}
