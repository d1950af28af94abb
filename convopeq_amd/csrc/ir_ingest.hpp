// ir_ingest.hpp -- the three steps of cpq_ir_prepare (ir_ingest.cpp), for callers that put another transform between them:
// cpq_ir_prepare itself (the host's minimum-phase conversion) and cpq_ir_prepare_batch (engine_minphase.cpp: one device
// conversion over every IR of the batch).  Host only, no HIP.
#pragma once

#include "convopeq_mi355x.h"

namespace cpq {

// Step one: the call checks of cpq_ir_prepare, then trailing-silence trim, DC blocker, window, target length and fade-out into
// out->ir (doTrimStep).  out is zeroed first; on an error out->ir holds no memory.
int irPrepareTrim(const cpq_ir_buffer* loaded, double sampleRate, float targetIrLengthSec, int phaseMode, const cpq_ir_buffer* currentIr,
                  cpq_ir_prepared* out);
// Step two: a converted IR replaces the trimmed one only when it validates -- finite, peak above 1e-12 (LoaderThread.cpp:652-680).
// true: ir now holds converted's samples (both have ir's shape).
bool irPrepareAccept(const cpq_ir_buffer* converted, cpq_ir_buffer* ir);
// Step three: scale factor against the IR playing now, peak latency.  On an error out->ir is freed.
int irPrepareFinish(const cpq_ir_buffer* currentIr, double currentScale, cpq_ir_prepared* out);
// a few words for a step's error code
const char* irPrepareWhy(int rc);

}  // namespace cpq
