// tsdf_units.h -- the host half of ScalableTSDFVolume::Integrate's touched units: from the per-pixel unit boxes that
// touched_kernel (tsdf.hip) writes to the set of unit keys.  Host-only and free of HIP, so that a stand-alone driver
// (tests/cpp/tsdf_units_driver.cpp) runs it under the address and undefined-behaviour sanitizers.
//
// THE RULE (include/visma_icp.h; tests/tsdf_spec.py touched_units): a strided pixel touches no unit if its
// point has a coordinate that is not finite, or if either of its box indices floor((p -+ sdf_trunc) / unit length) lies
// outside +-2^30 on any axis.  The kernel decides that in f64 BEFORE any conversion to int and says so in `valid`; no index
// value means "no box".  expand_touched_boxes applies the index half of the rule again to whatever it is given, so that no
// array of boxes -- INT_MAX or INT_MIN bounds included -- makes its loops long or their counters overflow.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <set>

namespace visma {

constexpr int32_t kTsdfUnitIndexLimit = 1 << 30;         // a unit index lies in [-2^30, 2^30]

struct TouchedBox {
    int32_t lo[3], hi[3];                                // floor((p - sdf_trunc) / unit length), floor((p + sdf_trunc) / unit length)
    int32_t valid;                                       // 0: the pixel touches no unit (no depth, or THE RULE); lo, hi mean nothing then
};

inline bool tsdf_unit_index_in_range(int32_t v) { return v >= -kTsdfUnitIndexLimit && v <= kTsdfUnitIndexLimit; }

// every unit key lo <= k <= hi (per axis) of every valid box whose six indices are in range, once each, in lexicographic
// order.  An inverted box (hi < lo on an axis) has no keys.
inline std::set<std::array<int32_t, 3>> expand_touched_boxes(const TouchedBox *boxes, size_t n)
{
    std::set<std::array<int32_t, 6>> distinct;           // most pixels of a frame share their box with a neighbour
    for (size_t i = 0; i < n; i++) {
        const TouchedBox &b = boxes[i];
        if (!b.valid) continue;
        bool in_range = true;
        for (int a = 0; a < 3; a++) in_range = in_range && tsdf_unit_index_in_range(b.lo[a]) && tsdf_unit_index_in_range(b.hi[a]);
        if (in_range) distinct.insert({b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]});
    }
    std::set<std::array<int32_t, 3>> keys;
    for (const auto &q : distinct)                       // (64-bit counters: hi + 1 never wraps)
        for (int64_t x = q[0]; x <= q[3]; x++)
            for (int64_t y = q[1]; y <= q[4]; y++)
                for (int64_t z = q[2]; z <= q[5]; z++) keys.insert({(int32_t)x, (int32_t)y, (int32_t)z});
    return keys;
}

}  // namespace visma
