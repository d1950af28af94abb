// What the reference's MklFftEvaluator.h touches of JUCE beyond the noise shapers' needs, for tests/golden/score_probe.cpp only:
// the existing shim (../juce_shim/JuceHeader.h) as it stands, plus FloatVectorOperations::copy, DBG and the String that DBG's
// argument builds.  This directory comes first on the probe's include path, so <JuceHeader.h> is this file.
#pragma once
#define FloatVectorOperations FloatVectorOperationsOfTheShapers
#include "../juce_shim/JuceHeader.h"
#undef FloatVectorOperations
#define DBG(x) ((void)0)
namespace juce {
struct FloatVectorOperations : FloatVectorOperationsOfTheShapers {
    static void copy(double* d, const double* s, int n) { std::memcpy(d, s, sizeof(double) * (size_t)n); }
};
// MklFftEvaluator builds one inside DBG(), which expands to nothing
struct String {
    String() {}
    String(const char*) {}
    explicit String(int) {}
    String operator+(const String&) const { return {}; }
};
}  // namespace juce
