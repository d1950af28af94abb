// dither_design.cpp -- host side of the dither stage: prepare() of the reference's three deterministic noise shapers
// (src/FixedNoiseShaper.h:70-108, 299-342; src/Fixed15TapNoiseShaper.h:88-134, 344-426; src/LatticeNoiseShaper.h:26-66), their
// generators' seeds, and the stage itself, sequentially, in the reference's operation order (processSample / quantize of each
// header).  No GPU.
// killDenormal is the identity, as in the reference's release build (src/DspNumericPolicy.h:189-204).  The 4-tap header leaves
// the contraction of its feedback sum to its compiler: here, as everywhere in this project, nothing is contracted.  The lattice
// header fuses four terms of its feedback sum itself (computeFeedback's _mm256_fmadd_pd): those are std::fma here.
#include "host_design.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>

namespace cpq {

namespace {

constexpr int kPresets = 10;
constexpr double kPresetRates[kPresets] = { 44100.0, 48000.0, 88200.0, 96000.0, 176400.0, 192000.0, 352800.0, 384000.0, 705600.0, 768000.0 };
constexpr double kPresets4[kPresets][4] = {
    { 0.394958, 0.319775, 0.145569, 0.139697 }, { 0.460000, 0.280000, 0.170000, 0.090000 }, { 0.727810, 0.189547, 0.125028, -0.042385 },
    { 0.742333, 0.185474, 0.106133, -0.033940 }, { 0.775904, 0.126967, 0.043467, 0.053661 }, { 0.774132, 0.117440, 0.047291, 0.061137 },
    { 0.724647, 0.094403, 0.113208, 0.067743 }, { 0.714605, 0.097798, 0.124553, 0.063045 }, { 0.635851, 0.161114, 0.194506, 0.008529 },
    { 0.624827, 0.174509, 0.201424, -0.000760 } };
constexpr double kPresets15[kPresets][16] = {
    { 2.157553, -2.356649, 2.179194, -1.802605, 1.429476, -1.073975, 0.775233, -0.535496, 0.360294, -0.229526, 0.143225, -0.081483, 0.045992, -0.021109, 0.009877, 0.0 },
    { 2.172009, -2.313034, 2.092949, -1.698718, 1.304487, -0.946581, 0.645299, -0.415598, 0.251068, -0.141026, 0.072650, -0.033120, 0.012821, -0.004274, 0.001068, 0.0 },
    { 1.458665, -1.271063, 1.372588, -1.257752, 1.186326, -1.042666, 0.931875, -0.787020, 0.671068, -0.541164, 0.438950, -0.333234, 0.250772, -0.174640, 0.097295, 0.0 },
    { 1.366976, -1.123204, 1.234291, -1.119397, 1.063887, -0.931030, 0.838107, -0.707665, 0.608977, -0.492384, 0.404256, -0.308827, 0.236248, -0.167088, 0.096853, 0.0 },
    { 0.892356, -0.425055, 0.645737, -0.531778, 0.565511, -0.483687, 0.474500, -0.404025, 0.379228, -0.317474, 0.286683, -0.233505, 0.199702, -0.166141, 0.117948, 0.0 },
    { 0.842437, -0.356337, 0.593464, -0.477529, 0.519248, -0.440863, 0.438827, -0.372969, 0.354221, -0.297057, 0.271334, -0.222591, 0.192842, -0.164283, 0.119255, 0.0 },
    { 0.576947, -0.000943, 0.355358, -0.225398, 0.306449, -0.241465, 0.271718, -0.228634, 0.237327, -0.205281, 0.201703, -0.179310, 0.166143, -0.176849, 0.142236, 0.0 },
    { 0.550200, 0.035746, 0.334748, -0.202925, 0.287573, -0.223403, 0.255932, -0.214959, 0.225551, -0.196308, 0.194281, -0.175339, 0.163224, -0.180050, 0.145728, 0.0 },
    { 0.403358, 0.274330, 0.229984, -0.085257, 0.190310, -0.131467, 0.169688, -0.142598, 0.154703, -0.144947, 0.142117, -0.148598, 0.132904, -0.195545, 0.151017, 0.0 },
    { 0.390229, 0.306061, 0.221612, -0.075413, 0.182734, -0.125438, 0.162912, -0.138648, 0.149015, -0.142960, 0.137870, -0.149116, 0.130580, -0.202133, 0.152692, 0.0 } };
// FixedNoiseShaper::rngState, channels 0 and 1
constexpr unsigned long long kSeeds4[2][4] = {
    { 0x123456789ABCDEF0ULL, 0xFEDCBA9876543210ULL, 0x0123456789ABCDEFULL, 0xEFCDAB8967452301ULL },
    { 0x89ABCDEF01234567ULL, 0x76543210FEDCBA98ULL, 0xABCDEF0123456789ULL, 0x67452301EFCDAB89ULL } };

// kDefaultAdaptiveNoiseShaperCoeffs (src/audioengine/AudioEngine.Processing.DSPCoreLifecycle.cpp:32-35)
constexpr double kAdaptiveDefault[kLatticeOrder] = { -0.003796, -0.006752, 0.008418, -0.010546, 0.004716, -0.007624, -0.020750, -0.002049, -0.003632 };

// selectPresetWithInterpolation: a NaN rate matches no branch and leaves the caller's zeros (preset 0, t = 0)
void selectPreset(double rate, int& lo, int& hi, double& t)
{
    lo = hi = 0;
    t = 0.0;
    if (rate <= kPresetRates[0]) return;
    if (rate >= kPresetRates[kPresets - 1]) { lo = hi = kPresets - 1; return; }
    for (int i = 0; i + 1 < kPresets; ++i)
        if (rate >= kPresetRates[i] && rate < kPresetRates[i + 1]) {
            lo = i;
            hi = i + 1;
            t = (rate - kPresetRates[i]) / (kPresetRates[i + 1] - kPresetRates[i]);
            return;
        }
}

unsigned long long splitmix64(unsigned long long& state)
{
    unsigned long long z = (state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

unsigned long long rotl(unsigned long long x, int k) { return (x << k) | (x >> (64 - k)); }

double uniform(unsigned long long s[4])
{
    const unsigned long long result = rotl(s[0] + s[3], 23) + s[0];
    const unsigned long long t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl(s[3], 45);
    return (double)(result >> 11) * (1.0 / 9007199254740992.0);
}

double finiteOrZero(double v) { return std::isfinite(v) ? v : 0.0; }

}  // namespace

bool ditherDesign(double rate, int shaper, int bits, double coeffs[kDitherMaxOrder], double* scale)
{
    const int order = ditherOrder(shaper);
    if (!order || bits < 1 || bits > 32) return false;
    *scale = 1.0 / std::ldexp(1.0, bits - 1);
    if (shaper == CPQ_DITHER_ADAPTIVE9) {       // LatticeNoiseShaper::prepare(bitDepth) takes no rate
        for (int i = 0; i < kDitherMaxOrder; ++i) coeffs[i] = i < kLatticeOrder ? kAdaptiveDefault[i] : 0.0;
        return true;
    }
    int lo, hi;
    double t;
    selectPreset(rate, lo, hi, t);
    for (int i = 0; i < kDitherMaxOrder; ++i) {
        if (i >= order) { coeffs[i] = 0.0; continue; }
        const double cLow = order == 4 ? kPresets4[lo][i] : kPresets15[lo][i], cHigh = order == 4 ? kPresets4[hi][i] : kPresets15[hi][i];
        coeffs[i] = t < 1e-12 ? cLow : t > 1.0 - 1e-12 ? cHigh : (1.0 - t) * cLow + t * cHigh;
    }
    // FixedNoiseShaper::setCoefficients refuses a set whose sum is off 1.0 by more than 1e-12 (the 44.1, 176.4, 352.8 and 384 kHz
    // presets sum to 1 -+ 1e-6) and keeps what it had: for a shaper fresh from its constructor, as every design here is, the
    // 48 kHz preset
    if (order == 4 && std::fabs(coeffs[0] + coeffs[1] + coeffs[2] + coeffs[3] - 1.0) > 1.0e-12)
        for (int i = 0; i < 4; ++i) coeffs[i] = kPresets4[1][i];
    return true;
}

void ditherSeed(int shaper, double rate, int bits, int ch, unsigned long long s[4])
{
    if (shaper != CPQ_DITHER_FIXED15) { std::memcpy(s, kSeeds4[ch & 1], sizeof(kSeeds4[0])); return; }
    const double safeRate = (rate > 0.0 && std::isfinite(rate)) ? rate : 48000.0;
    unsigned long long seed;
    std::memcpy(&seed, &safeRate, sizeof(seed));
    seed ^= (unsigned long long)bits << 32;
    seed ^= 0xD1B54A32D192ED03ULL;
    unsigned long long stream = seed ^ (0x9E3779B97F4A7C15ULL * (unsigned long long)(ch + 1));
    for (int i = 0; i < 4; ++i) s[i] = splitmix64(stream);
    if ((s[0] | s[1] | s[2] | s[3]) == 0ULL) s[0] = 1ULL;
}

void ditherClampAdaptive(const double* k, int n, double out[kLatticeOrder])
{
    for (int i = 0; i < kLatticeOrder; ++i) {
        const double v = i < n ? k[i] : 0.0;
        out[i] = !std::isfinite(v) ? 0.0 : v > 0.85 ? 0.85 : v < -0.85 ? -0.85 : v;
    }
}

bool DitherHost::configure(double rate, int shaperId, int bitDepth)
{
    double c[kDitherMaxOrder], sc;
    if (!ditherDesign(rate, shaperId, bitDepth, c, &sc)) return false;
    shaper = shaperId;
    order = ditherOrder(shaperId);
    bits = bitDepth;
    std::memcpy(coeffs, c, sizeof(c));
    scale = sc;
    invScale = std::ldexp(1.0, bits - 1);
    for (int ch = 0; ch < 2; ++ch) ditherSeed(shaper, rate, bits, ch, rng[ch]);
    reset();
    return true;
}

void DitherHost::prepare(double rate)
{
    if (!order) return;
    if (shaper != CPQ_DITHER_ADAPTIVE9) ditherDesign(rate, shaper, bits, coeffs, &scale);
    if (shaper == CPQ_DITHER_FIXED15)
        for (int ch = 0; ch < 2; ++ch) ditherSeed(shaper, rate, bits, ch, rng[ch]);
    reset();
}

void DitherHost::reset() { std::memset(err, 0, sizeof(err)); }

bool DitherHost::setAdaptiveCoeffs(const double* k, int n)
{
    if (shaper != CPQ_DITHER_ADAPTIVE9 || n < 0 || n > kLatticeOrder || (n > 0 && !k)) return false;
    ditherClampAdaptive(k, n, coeffs);
    reset();
    return true;
}

// LatticeNoiseShaper::processStereoBlock.  Its closing clampStateSIMD (+-1e12) cannot act on states that advanceState already
// holds to +-2 and is left out
static void latticeProcess(DitherHost& h, double* const rows[2], int n, double headroom)
{
    const double scale = h.scale, invScale = h.invScale;
    const double minV = -1.0, maxV = 1.0 - (1.0 / invScale), lim = 2.0 * scale;
    for (int ch = 0; ch < 2; ++ch) {
        double* st = h.err[ch];
        const double* c = h.coeffs;
        unsigned long long* rng = h.rng[ch];
        for (int i = 0; i < n; ++i) {
            const double x = rows[ch][i] * headroom;
            double p[4];
            for (int j = 0; j < 4; ++j) p[j] = std::fma(st[4 + j], c[4 + j], st[j] * c[j]);
            const double fb = ((p[0] + p[2]) + (p[1] + p[3])) + st[8] * c[8];
            const double y = x + fb;
            double v = y;                                       // a NaN passes both comparisons
            if (v < minV) v = minV;
            else if (v > maxV) v = maxV;
            const double u1 = uniform(rng);
            const double u2 = uniform(rng);
            v += (u1 + u2 - 1.0) * scale;
            const double q = std::nearbyint(v * invScale);
            const double minQ = -invScale, maxQ = invScale - 1.0;
            const double yq = (q < minQ ? minQ : (maxQ < q ? maxQ : q)) * scale;       // std::clamp: a NaN stays
            const double error = finiteOrZero(yq - y);
            double f = error < -lim ? -lim : (lim < error ? lim : error);
            for (int k = 0; k < kLatticeOrder; ++k) {           // advanceState
                const double b = st[k];
                const double nf = f + c[k] * b;
                const double nb = c[k] * f + b;
                st[k] = nb < -2.0 ? -2.0 : (2.0 < nb ? 2.0 : nb);
                f = nf;
            }
            rows[ch][i] = yq;
        }
    }
}

void DitherHost::process(double* l, double* r, int n, double headroom)
{
    if (!order || n <= 0) return;
    double* rows[2] = { l, r };
    const double minV = -1.0, maxV = 1.0 - (1.0 / invScale), lim = 2.0 * scale;
    if (shaper == CPQ_DITHER_ADAPTIVE9) { latticeProcess(*this, rows, n, headroom); return; }
    for (int ch = 0; ch < 2; ++ch) {
        double* e = err[ch];
        for (int i = 0; i < n; ++i) {
            const double x = rows[ch][i] * headroom;
            double fb;
            if (order == 4) {
                fb = coeffs[0] * e[0] + coeffs[1] * e[1] + coeffs[2] * e[2] + coeffs[3] * e[3];
            } else {
                fb = 0.0;
                for (int k = 0; k < 16; ++k) fb += coeffs[k] * e[k];
            }
            const double y = x - fb;
            double v = order == 4 ? finiteOrZero(y) : y;
            if (v < minV) v = minV;
            else if (v > maxV) v = maxV;
            const double u1 = uniform(rng[ch]);
            const double u2 = uniform(rng[ch]);
            v += (u1 + u2 - 1.0) * scale;
            const double q = std::nearbyint(v * invScale);      // round to nearest even: the default rounding mode
            double yq, stored;
            if (order == 4) {
                yq = finiteOrZero(q * scale);
                const double error = yq - y;
                stored = error < -lim ? -lim : (lim < error ? lim : error);     // std::clamp: a NaN stays
                stored = finiteOrZero(stored);
            } else {
                const double minQ = -invScale, maxQ = invScale - 1.0;
                yq = (q < minQ ? minQ : (maxQ < q ? maxQ : q)) * scale;         // std::clamp: a NaN stays
                const double error = yq - y;
                stored = error > -lim ? error : -lim;                           // max_sd: a NaN gives the second operand
                stored = stored < lim ? stored : lim;                           // min_sd
                stored = finiteOrZero(stored);
            }
            for (int k = order - 1; k > 0; --k) e[k] = e[k - 1];
            e[0] = stored;
            rows[ch][i] = yq;
        }
    }
}

}  // namespace cpq

extern "C" {

int32_t cpq_dither_design(double rate, int32_t shaper, int32_t bitDepth, double coeffs[16], double* scale)
{
    if (!coeffs || !scale) return CPQ_ERR_INVALID_ARG;
    return cpq::ditherDesign(rate, shaper, bitDepth, coeffs, scale) ? CPQ_OK : CPQ_ERR_INVALID_ARG;
}

}  // extern "C"
