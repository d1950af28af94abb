// Records what the reference's own CmaEsOptimizer computes, for tests/golden/learn_ref.npz (make_learn_ref.py drives it).  Build,
// with REF the reference's source tree:
//   g++ -std=c++20 -O2 -ffp-contract=off -Itests/golden/juce_shim -I$REF/src tests/golden/learn_probe.cpp -o learn_probe
//   learn_probe <script> <out>
// script: whitespace-separated commands, numbers as C99 hex floats:
//   params <sigmaMin> <sigmaMax> <covRetentionTarget> <covRetentionStep>    setParams
//   init <9 values>                                                         initFromParcor
//   load <9 mean> <45 cov> <sigma>                                          deserializeFrom
//   seed <integer>                                                          setSeed, and the twin generator the same
//   dump                                                                    out += serializeTo (9 + 45 + 1 doubles)
//   gen <18 fitness>                                                        out += serializeTo, z, candidates, fitness, serializeTo
// sample() draws from a std::normal_distribution constructed in the call; the twin std::mt19937, seeded alike, gives a
// distribution constructed here the same words, so z is exactly what sample() drew.
#include <JuceHeader.h>
#include "CmaEsOptimizer.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    std::vector<double> out;
    auto opt = std::make_unique<CmaEsOptimizer>();
    std::mt19937 twin;
    auto number = [&in]() { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); };
    auto dump = [&]() {
        double m[9], c[45], s;
        opt->serializeTo(m, c, s);
        out.insert(out.end(), m, m + 9);
        out.insert(out.end(), c, c + 45);
        out.push_back(s);
    };
    std::string cmd;
    while (in >> cmd) {
        if (cmd == "params") {
            CmaEsOptimizer::Params p;
            p.sigmaMin = number(); p.sigmaMax = number(); p.covRetentionTarget = number(); p.covRetentionStep = number();
            opt->setParams(p);
        } else if (cmd == "init") {
            double k[9];
            for (double& v : k) v = number();
            opt->initFromParcor(k);
        } else if (cmd == "load") {
            double m[9], c[45];
            for (double& v : m) v = number();
            for (double& v : c) v = number();
            opt->deserializeFrom(m, c, number());
        } else if (cmd == "seed") {
            std::string t; in >> t;
            const unsigned long long s = std::strtoull(t.c_str(), nullptr, 10);
            opt->setSeed(s);
            twin.seed(static_cast<std::mt19937::result_type>(s));
        } else if (cmd == "dump") {
            dump();
        } else if (cmd == "gen") {
            double f[18], cand[18][9];
            for (double& v : f) v = number();
            dump();
            opt->sample(cand);
            std::normal_distribution<double> nd(0.0, 1.0);
            for (int i = 0; i < 18 * 9; ++i) out.push_back(nd(twin));
            for (auto& row : cand) out.insert(out.end(), row, row + 9);
            out.insert(out.end(), f, f + 18);
            opt->update(cand, f);
            dump();
        } else {
            return 3;
        }
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    std::fclose(f);
    return 0;
}
