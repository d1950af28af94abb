// The few names of JUCE that the reference's noise-shaper headers touch, for tests/golden/dither_probe.cpp only.
#pragma once
#include <cstring>
#define jassert(x) ((void)0)
namespace juce {
struct FloatVectorOperations {
    static void clear(double* d, int n) { std::memset(d, 0, sizeof(double) * (size_t)n); }
};
// the shapers only push diagnostics into it; nothing here reads them back
struct AbstractFifo {
    explicit AbstractFifo(int) {}
    void reset() {}
    void prepareToWrite(int, int& s1, int& n1, int& s2, int& n2) { s1 = n1 = s2 = n2 = 0; }
    void finishedWrite(int) {}
};
}  // namespace juce
