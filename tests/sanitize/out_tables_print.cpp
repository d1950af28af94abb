// Prints what the DC kernel is given for a list of rates (convopeq_amd/csrc/out_design.cpp): per rate and section one line
//   <rate> <section> <72 hex floats of outSectionTable>
// for tests/test_out_edges_cpu.py, which holds the lines to tests/out_edge_inputs.py bit for bit.
#include "host_design.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; ++i) {
        const double rate = std::atof(argv[i]);
        double alpha[2], release, tab[cpq::kOutSectionDoubles];
        cpq::outDesign(rate, alpha, &release);
        for (int s = 0; s < 2; ++s) {
            cpq::outSectionTable(alpha[s], tab);
            std::printf("%.1f %d", rate, s);
            for (int k = 0; k < cpq::kOutSectionDoubles; ++k) std::printf(" %a", tab[k]);
            std::printf("\n");
        }
    }
    return 0;
}
