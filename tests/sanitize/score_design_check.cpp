// Stand-alone check of the shaper scorer's host code (convopeq_amd/csrc/score_design.cpp: scoreTables, scoreSelectSegments,
// scoreRngTable and the candidate tests), built with the address and undefined-behaviour sanitizers and run as a program of its
// own on exactly-sized heap rows -- against a dump written by tests/test_score_model_cpu.py from tests/score_model.py:
//   tables <rate> <4 bins> then weight, bark, athDb, width (2049 each), ultraShare, flatWeight, hfWeight, weightSum as hex bit
//          patterns, then band and range (2049 ints each)
//   audio <n> <nSeg> <4 counts>, then 2 n input doubles (hex), then per segment start level type gain(hex)
//   rng <count>, then count x 2 x 4 words (hex)
#include "host_design.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <limits>
#include <vector>

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static bool readDoubles(FILE* f, std::vector<double>& v)
{
    for (auto& x : v) {
        uint64_t bits;
        if (std::fscanf(f, "%" SCNx64, &bits) != 1) return false;
        std::memcpy(&x, &bits, sizeof(x));
    }
    return true;
}
static bool readInts(FILE* f, std::vector<int>& v)
{
    for (auto& x : v) if (std::fscanf(f, "%d", &x) != 1) return false;
    return true;
}
static bool same(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

static unsigned long long rotl(unsigned long long x, int k) { return (x << k) | (x >> (64 - k)); }
static void draw(unsigned long long s[4])
{
    const unsigned long long t = s[1] << 17;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
}

int main(int argc, char** argv)
{
    int nTables = 0, nAudio = 0, nRng = 0;
    FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
    CHECK(f != nullptr);
    char word[16];
    while (f && std::fscanf(f, " %15s", word) == 1) {
        if (!std::strcmp(word, "tables")) {
            double rate;
            int bins[4];
            if (std::fscanf(f, "%lf %d %d %d %d", &rate, &bins[0], &bins[1], &bins[2], &bins[3]) != 5) { CHECK(!"short tables"); break; }
            std::vector<double> w(cpq::kScoreBins), bark(w), ath(w), width(w), sc(4);
            std::vector<int> band(cpq::kScoreBins), range(band);
            if (!readDoubles(f, w) || !readDoubles(f, bark) || !readDoubles(f, ath) || !readDoubles(f, width) || !readDoubles(f, sc) ||
                !readInts(f, band) || !readInts(f, range)) { CHECK(!"short tables"); break; }
            cpq::ScoreTables t;
            CHECK(cpq::scoreTables(rate, t));
            CHECK(same(t.weight, w) && same(t.bark, bark) && same(t.athDb, ath) && same(t.width, width));
            CHECK(t.band == band && t.range == range);
            CHECK(t.flatStart == bins[0] && t.flatEnd == bins[1] && t.highStart == bins[2] && t.ultraStart == bins[3]);
            CHECK(t.ultraShare == sc[0] && t.flatWeight == sc[1] && t.hfWeight == sc[2] && t.weightSum == sc[3]);
            CHECK(t.bandStart[0] == 0 && t.bandStart[cpq::kScoreBands] == cpq::kScoreBins);
            for (int b = 0; b < cpq::kScoreBands; ++b)
                for (int i = t.bandStart[b]; i < t.bandStart[b + 1]; ++i) CHECK(t.band[i] == b);
            CHECK(t.spreadTonal.size() == 1601 && t.spreadNoise[800] == 0.0 && t.spreadTonal[1600] == -27.0 * (-8.0 + 1600.0 * 0.01));
            CHECK(t.athPow.size() == (size_t)cpq::kScoreBins && t.thrSpread[0] == std::pow(10.0, -12.0 / 10.0));
            ++nTables;
        } else if (!std::strcmp(word, "audio")) {
            int n, nSeg, counts[4];
            if (std::fscanf(f, "%d %d %d %d %d %d", &n, &nSeg, &counts[0], &counts[1], &counts[2], &counts[3]) != 6) { CHECK(!"short audio"); break; }
            std::vector<double> l((size_t)n), r((size_t)n);             // exact sizes: a read past n is a sanitizer report
            if (!readDoubles(f, l) || !readDoubles(f, r)) { CHECK(!"short audio"); break; }
            cpq::ScoreSegment seg[cpq::kScoreMaxSegments];
            int got[4];
            CHECK(cpq::scoreSelectSegments(l.data(), r.data(), n, seg, got) == nSeg);
            CHECK(std::memcmp(got, counts, sizeof(got)) == 0);
            for (int i = 0; i < nSeg; ++i) {
                int start, level, type;
                std::vector<double> gain(1);
                if (std::fscanf(f, "%d %d %d", &start, &level, &type) != 3 || !readDoubles(f, gain)) { CHECK(!"short segment"); break; }
                CHECK(seg[i].start == start && seg[i].level == level && seg[i].type == type && seg[i].gain == gain[0]);
            }
            ++nAudio;
        } else if (!std::strcmp(word, "rng")) {
            int count;
            if (std::fscanf(f, "%d", &count) != 1) { CHECK(!"short rng"); break; }
            std::vector<double> raw((size_t)count * 8);
            if (!readDoubles(f, raw)) { CHECK(!"short rng"); break; }
            const unsigned long long start[2][4] = {
                { 0x123456789ABCDEF0ULL, 0xFEDCBA9876543210ULL, 0x0123456789ABCDEFULL, 0xEFCDAB8967452301ULL },
                { 0x89ABCDEF01234567ULL, 0x76543210FEDCBA98ULL, 0xABCDEF0123456789ULL, 0x67452301EFCDAB89ULL } };
            std::vector<unsigned long long> table;
            cpq::scoreRngTable(start, count, table);
            CHECK(table.size() == raw.size() && std::memcmp(table.data(), raw.data(), raw.size() * 8) == 0);
            ++nRng;
        } else { CHECK(!"unknown record"); break; }
    }
    if (f) std::fclose(f);
    CHECK(nTables == 3 && nAudio >= 4 && nRng == 1);
    {   // both modes' indices against word-by-word stepping, from a start state of the caller's
        const unsigned long long start[2][4] = { { 1, 2, 3, 4 }, { 5, 6, 7, 8 } };
        const int nSeg = 3, nCand = 2;
        std::vector<unsigned long long> table;
        cpq::scoreRngTable(start, nCand * nSeg, table);
        for (int ch = 0; ch < 2; ++ch) {
            unsigned long long s[4];
            std::memcpy(s, start[ch], sizeof(s));
            for (int j = 0; j < nCand * nSeg; ++j) {
                const int c = j / nSeg, sg = j % nSeg;
                CHECK(cpq::scoreRngIndex(CPQ_SCORE_RNG_CHAINED, c, nSeg, sg) == j && cpq::scoreRngIndex(CPQ_SCORE_RNG_FRESH, c, nSeg, sg) == sg);
                CHECK(std::memcmp(&table[((size_t)j * 2 + ch) * 4], s, sizeof(s)) == 0);
                for (int k = 0; k < 2 * cpq::kScoreLen; ++k) draw(s);
            }
        }
        cpq::scoreRngTable(start, 0, table);
        CHECK(table.empty());
    }
    {   // selection edges: too short, all quiet, null rows; more than kScoreRecent samples use the last ones
        std::vector<double> z(4095, 0.25), q(9000, 1.0e-6);
        cpq::ScoreSegment seg[cpq::kScoreMaxSegments];
        int counts[4];
        CHECK(cpq::scoreSelectSegments(z.data(), z.data(), 4095, seg, counts) == 0 && counts[0] == 0 && counts[3] == 0);
        CHECK(cpq::scoreSelectSegments(q.data(), q.data(), 9000, seg, counts) == 0);
        CHECK(cpq::scoreSelectSegments(nullptr, nullptr, 0, seg, counts) == 0);
        std::vector<double> big((size_t)cpq::kScoreRecent + 1000, 1.0e-7);
        for (size_t i = 1000; i < 1000 + 4096; ++i) big[i] = (i & 1) ? 0.5 : -0.5;     // the first window of the samples used
        CHECK(cpq::scoreSelectSegments(big.data(), big.data(), (int)big.size(), seg, counts) == 8);      // windows 0 and 2048 pass the gate
        CHECK(seg[0].start == 0 && seg[1].start == 2048 && seg[0].type == CPQ_SEGMENT_TONAL && seg[1].type == CPQ_SEGMENT_TONAL);
        CHECK(seg[0].gain == std::pow(10.0, -40.0 / 20.0) / 0.5 && seg[6].level == 3 && seg[6].gain == std::pow(10.0, -10.0 / 20.0) / 0.5);
    }
    {   // candidates
        const double ok[9] = { 0.99, -0.99, 0, 0, 0, 0, 0, 0, 0 }, bad[9] = { 0, 0, 0, 0, 0, 0, 0, 0, -1.0 };
        CHECK(cpq::scoreStable(ok, 9) && !cpq::scoreStable(bad, 9));
        const double raw[9] = { 0.0, 10.0, -10.0, 0.5, std::nan(""), std::numeric_limits<double>::infinity(), -0.25, 1.0e-3, -40.0 };
        double k[9];
        cpq::scoreMapRaw(raw, 0.85, k);
        CHECK(k[0] == 0.0 && k[1] == 0.85 && k[2] == -0.85 && k[3] == std::tanh(0.5) && k[4] == 0.0 && k[5] == 0.85 && k[8] == -0.85);
        CHECK(cpq::scoreAlpha(0) == 0.3 && cpq::scoreAlpha(1) == 0.5 && cpq::scoreAlpha(2) == 0.5 && cpq::scoreAlpha(3) == 0.7);
        cpq::ScoreTables t;
        CHECK(cpq::scoreTables(0.0, t) && t.rate == 1.0);      // configureForSampleRate's own floor
    }
    std::printf("score_design_check: %d tables, %d audio, %d rng, %d failed checks\n", nTables, nAudio, nRng, failed);
    return failed ? 1 : 0;
}
