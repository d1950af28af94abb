// The five names of Intel IPP that the reference's MklFftEvaluator.h touches, for tests/golden/score_probe.cpp only.
// ippsFFTFwd_RToCCS_64f here is the definition of the transform, X[k] = sum x[n] exp(-2 pi i n k / N) without scaling, evaluated
// in long double (twiddles from cosl / sinl of the reduced index, a radix-2 recursion on long double values) and rounded to
// double once at the end: the recorded spectra are the exact ones to about half an ulp, and IPP's own output -- like any other
// transform's -- differs from them by its own rounding only.
#pragma once
#include <cmath>
#include <complex>
#include <cstdlib>
#include <vector>

typedef double Ipp64f;
typedef unsigned char Ipp8u;
typedef int IppStatus;
typedef int IppHintAlgorithm;
enum { ippStsNoErr = 0 };
enum { IPP_FFT_NODIV_BY_ANY = 8 };
enum { ippAlgHintFast = 1 };
struct IppsFFTSpec_R_64f { int order; };

inline IppStatus ippsFFTGetSize_R_64f(int, int, IppHintAlgorithm, int* sizeSpec, int* sizeInit, int* sizeWork)
{
    *sizeSpec = (int)sizeof(IppsFFTSpec_R_64f);
    *sizeInit = 0;
    *sizeWork = 0;
    return ippStsNoErr;
}
inline Ipp8u* ippsMalloc_8u(int n) { return static_cast<Ipp8u*>(std::malloc((size_t)(n > 0 ? n : 1))); }
inline void ippsFree(void* p) { std::free(p); }
inline IppStatus ippsFFTInit_R_64f(IppsFFTSpec_R_64f** spec, int order, int, IppHintAlgorithm, Ipp8u* specBuf, Ipp8u*)
{
    *spec = reinterpret_cast<IppsFFTSpec_R_64f*>(specBuf);
    (*spec)->order = order;
    return ippStsNoErr;
}

namespace score_shim {
typedef std::complex<long double> cld;
inline void fft(std::vector<cld>& a)
{
    const size_t n = a.size();
    if (n == 1) return;
    std::vector<cld> even(n / 2), odd(n / 2);
    for (size_t i = 0; i < n / 2; ++i) { even[i] = a[2 * i]; odd[i] = a[2 * i + 1]; }
    fft(even);
    fft(odd);
    const long double step = -2.0L * 3.14159265358979323846264338327950288L / (long double)n;
    for (size_t k = 0; k < n / 2; ++k) {
        const cld w(cosl(step * (long double)k), sinl(step * (long double)k));
        const cld t = w * odd[k];
        a[k] = even[k] + t;
        a[k + n / 2] = even[k] - t;
    }
}
}  // namespace score_shim

// CCS: re0 im0 re1 im1 ... re(N/2) im(N/2)
inline IppStatus ippsFFTFwd_RToCCS_64f(const Ipp64f* src, Ipp64f* dst, const IppsFFTSpec_R_64f* spec, Ipp8u*)
{
    const size_t n = (size_t)1 << spec->order;
    std::vector<score_shim::cld> a(n);
    for (size_t i = 0; i < n; ++i) a[i] = score_shim::cld((long double)src[i], 0.0L);
    score_shim::fft(a);
    for (size_t k = 0; k <= n / 2; ++k) {
        dst[2 * k] = (double)a[k].real();
        dst[2 * k + 1] = (double)a[k].imag();
    }
    return ippStsNoErr;
}
