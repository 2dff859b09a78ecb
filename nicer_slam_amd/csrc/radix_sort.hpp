// radix_sort.hpp -- the stable LSD radix argsort of map_tail.hip (k_radix_hist / k_radix_scatter), for other translation units.
#pragma once
#include <cstdint>
#include "../../include/nicer_slam_amd.h"

namespace nsa {

// order[0, P) = the stable argsort of keys[0][0, P) by bits [shift0, shift0 + 8 * passes) (equal digits keep their index order).
// keys[0] is the input and, with keys[1], a ping-pong buffer (both P words; overwritten); tmp P words; counts 256 * 256 words.
// Launches 2 * passes kernels on `stream`; nothing is allocated or synchronised.  The caller brackets it with
// launch_begin() / launch_end() (or reads hipGetLastError() itself).  P <= 2^31 - 1.
void radix_argsort(uint32_t* const keys[2], uint32_t* tmp, uint32_t* order, uint32_t* counts, uint32_t P, uint32_t shift0,
                   uint32_t passes, nsa_stream_t stream);

constexpr uint32_t kRadixCountWords = 256u * 256u;      // counts[nb][256], nb <= 256 (map_tail.hip: radix_geometry)

}  // namespace nsa
