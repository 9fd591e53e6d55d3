// The modified Bessel function I0 of the Kaiser windows (the resampler's prototype and the meter's true-peak interpolator), host only.
#pragma once

namespace fmd {

// 1 + sum over k >= 1 of prod_{m <= k} (x / (2 m))^2, summed in k order until a term falls under 1e-18 of the sum
inline double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; k++) { term *= (x / (2.0 * k)) * (x / (2.0 * k)); sum += term; if (term < 1e-18 * sum) break; }
    return sum;
}

}  // namespace fmd
