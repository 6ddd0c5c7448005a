// held_rules.hpp -- what each held product of a context is made from: the one place in C++ that says so (the table is DESIGN.md
// 4.5a).  A held product is a raster, sometimes with records, that stays on the device outside mhip_raster until a write of
// something it was made from drops it.  Pure rules: no HIP, no buffers, no context -- tools/held_rules_check.cpp walks them on the
// host.  A feature that adds a held product adds an enumerator and its line in held_made_from (and in held_goes_with, if it is made
// from another product) here, and a row in ctx.hip's HELD table.
#pragma once
#include <cstdint>

#include "../../include/malstroem_hip.h"

namespace mh {

enum HeldProduct { HP_WETAT, HP_FLOWDIST, HP_TRAVELTIME, HP_HAND, HP_REACHCATCH, HP_INUNDATION, HP_ZONES, HP_SEALEVEL, HP_SEADEPTH, HP_SEACLASS, HP_COUNT_ };

// what a rule depends on beside the product: the elevation raster a hand was made from (FILLED or DEM), and whether the call read labels
constexpr int HELD_V_LABELS = 1 << 8;
constexpr int held_variant(int source, bool labels) { return source | (labels ? HELD_V_LABELS : 0); }

constexpr uint32_t held_bit(int k) { return 1u << k; }

// the rasters (a mask over mhip_raster) whose write drops `product`
constexpr uint32_t held_made_from(int product, int variant)
{
    const uint32_t labels = (variant & HELD_V_LABELS) ? held_bit(MHIP_R_LABELS) : 0;
    switch (product) {
    case HP_WETAT: return held_bit(MHIP_R_DEPTHS) | held_bit(MHIP_R_LABELS);
    case HP_FLOWDIST: return held_bit(MHIP_R_FLOWDIR) | held_bit(MHIP_R_LABELS);
    case HP_TRAVELTIME:      // (ACCUM also when the call read none: one rule for the four)
        return held_bit(MHIP_R_FLOWDIR) | held_bit(MHIP_R_LABELS) | held_bit(MHIP_R_FILLED) | held_bit(MHIP_R_ACCUM);
    case HP_HAND: return held_bit(MHIP_R_FLOWDIR) | held_bit(MHIP_R_ACCUM) | held_bit(variant & (HELD_V_LABELS - 1)) | labels;
    case HP_REACHCATCH: return held_bit(MHIP_R_FLOWDIR) | held_bit(MHIP_R_ACCUM) | labels;
    case HP_SEALEVEL: return held_bit(MHIP_R_DEM);
    default: return 0;      // INUNDATION, SEADEPTH, SEACLASS: with what they were made from, below; ZONES: they come from outside
    }
}

// the products (a mask over HeldProduct) that `product` was made from: dropping one of them for any reason, a new call of its own
// entry point included, drops `product`
constexpr uint32_t held_goes_with(int product)
{
    switch (product) {
    case HP_INUNDATION: return held_bit(HP_HAND) | held_bit(HP_REACHCATCH);
    case HP_SEADEPTH: case HP_SEACLASS: return held_bit(HP_SEALEVEL);
    default: return 0;
    }
}

// what a write of raster `which` counts as: a new DEM takes every other raster away, so it is a write of each of them
constexpr uint32_t held_write_mask(int which) { return which == MHIP_R_DEM ? held_bit(MHIP_R_COUNT_) - 1 : held_bit(which); }

}  // namespace mh
