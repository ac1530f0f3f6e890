// colour_lut.h -- setColor as a 256-entry table of packed (r | r_ << 8) channel pairs, one table per
// C3H_COLOR_* mode (color_chlac.hpp:148-179).  Plain C++: the context (capi.hip) uploads it, the
// host check of the packed rows (tests/packed_rows_check.cpp) reads it.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/c3hlac_mi355x.h"

namespace c3h {

inline void host_lut(int color_mode, uint32_t* out) {
  const float angle_norm = M_PI / 510;  // color_chlac/include/color_chlac/color_chlac.h:9
  for (int v = 0; v < 256; ++v) {
    const float a = v * angle_norm;
    int s, c;
    if (color_mode == C3H_COLOR_CHLAC) {  // ColorCHLAC: r_ = 255 - r
      s = v;
      c = 255 - v;
    } else if (color_mode == C3H_COLOR_C3_DOUBLE) {
      s = (int)(255 * std::sin((double)a));
      c = (int)(255 * std::cos((double)a));
    } else {
      s = (int)(255 * sinf(a));
      c = (int)(255 * cosf(a));
    }
    out[v] = (uint32_t)s | ((uint32_t)c << 8);
  }
}

}  // namespace c3h
