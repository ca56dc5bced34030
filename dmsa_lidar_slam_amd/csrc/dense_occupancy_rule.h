// dense_occupancy_rule.h — M5 and M6's coordinate of include/dmsa_dense_occupancy.h, stated once for the device kernels
// (csrc/dense_occupancy.hip) and for the host-only call dmsa_dense_occupancy_state (csrc/dense_occupancy_text.cpp), as dense_carve_walk.h is
// for T2-T5.  Integers and one double product; every translation unit that includes it is built with -ffp-contract=off.
#pragma once
#include <cstdint>

#include "dense_carve_walk.h"

namespace dmsa {

constexpr uint32_t kOccupancyUnknown = 0, kOccupancyFree = 1, kOccupancyOccupied = 2;

// M5: the four thresholds lie in [1, 2^20] and the counters below 2^27, so each product is below 2^47
DMSA_CARVE_HD uint32_t occupancy_state(const uint32_t min_hits, const uint32_t min_passes, const uint32_t occ_num, const uint32_t occ_den, const uint32_t hits,
                                       const uint32_t passes) {
    const uint64_t against = (uint64_t)passes * (uint64_t)occ_den, in_favour = (uint64_t)hits * (uint64_t)occ_num;
    if (hits >= min_hits && against <= in_favour) return kOccupancyOccupied;
    return passes >= min_passes ? kOccupancyFree : kOccupancyUnknown;
}
// M6: the centre of cell c on one axis, rounded once
DMSA_CARVE_HD float occupancy_centre(const int32_t c, const double cell) { return (float)(((double)c + 0.5) * cell); }

}  // namespace dmsa
