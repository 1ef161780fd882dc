// What forms.hip (include/jaicov_forms.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devbuf.h"

namespace jaicov {

// work buffers of jaicov_form_fit and jaicov_surf_fit (include/jaicov_surfaces.h), kept by the engine (they only grow)
struct FormState {
    DevBuf<int32_t> tab;       // type [n] | begin [n + 1] | status bits of the host [n] | point [M] | columns [3 M] | status [n] | member status [M]
    DevBuf<double> out;        // out [20 n] | qpp [28 n] | member_out [7 M] | start rows [7 n] (jaicov_surf_fit)
};

}  // namespace jaicov
