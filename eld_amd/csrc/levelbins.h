// levelbins.h -- the signal bins shared by pairstats.hip (error versus signal level) and burst.hip (photon-transfer sums): DESIGN.md sec. 19.
#pragma once
#include "common.h"

constexpr int PS_NB = 61;                        // bins: 0, 1..7, quarter octaves 8..59, saturated 60
static_assert(PS_NB == ELD_PAIRSTATS_BINS, "the header names the bin count");

// code = the site's code (the saturated bin is chosen by code >= white), s = code - black of its cell
__device__ __forceinline__ int bin_of(int code, int s, int white) {
    if (code >= white) return PS_NB - 1;
    if (s <= 0) return 0;
    if (s < 8) return s;
    const int o = 31 - __clz(s);
    return 8 + 4 * (o - 3) + ((s >> (o - 2)) & 3);
}
