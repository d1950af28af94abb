// Stands in for Intel MKL's header where the reference's MklFftEvaluator.h includes it: that header uses nothing of MKL itself
// (its transform is IPP's, see ipp.h beside this file).  For tests/golden/score_probe.cpp only.
#pragma once
