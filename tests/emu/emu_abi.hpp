// TEST INFRASTRUCTURE: what every CPU twin of a C-ABI entry point shares.  A twin `emu_x` stands in for `atr_x` of
// include/atropos_hip.h under the test-suite's backend (tests/emu/backend.py), which calls it through the product's
// own wrappers and prototypes (atropos_amd/_lib.py).  So it takes exactly atr_x's parameters -- the scratch and the
// stream included, which a twin ignores -- and says so right after its definition:
//
//     int emu_clip_batch(const atr_fastq_record *, int32_t *begin, ..., void *) { ... }
//     EMU_TWIN(clip_batch);
//
// A signature that drifts from the header then fails to compile instead of reading stack garbage.
#ifndef EMU_ABI_HPP
#define EMU_ABI_HPP

#include <type_traits>

#include "atropos_hip.h"

#define EMU_TWIN(name)                                                                          \
    static_assert(std::is_same<decltype(&emu_##name), decltype(&atr_##name)>::value,            \
                  "emu_" #name " must take the parameters of atr_" #name " (include/atropos_hip.h)")

#endif
