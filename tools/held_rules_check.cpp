// held_rules_check.cpp -- the rules of malstroem_amd/csrc/held_rules.hpp as text, for tests/test_held_rules.py to compare with the
// table of DESIGN.md 4.5a (tests/_ctx_shadow.py).  For every raster written x every held product x every variant of how the product
// was made (the elevation source of a hand: filled or dem; labels read or not) one line
//   <raster written> <product> <source>:<labels|nolabels> <dropped|survives>
// where "dropped" is the direct rule -- held_write_mask meets held_made_from -- or the cascade: a product that held_goes_with says it
// was made from is dropped by that write.  Then, for every pair of products, what a drop of the first for any reason -- a new call of
// its own entry point included -- does to the second:
//   call <product> <other product> <dropped|survives>
// Build and run (no GPU, no HIP):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I malstroem_amd/csrc tools/held_rules_check.cpp -o build/held_rules_check
//   build/held_rules_check
#include <cstdio>
#include <initializer_list>

#include "held_rules.hpp"

using namespace mh;

static const char *const RASTER[] = {"dem", "filled", "depths", "noflat", "flowdir", "accum", "labels", "watersheds", "ngdist", "finaldepths"};
static const char *const PRODUCT[] = {"wet_at", "flow_distance", "travel_time", "hand", "reach_catchments", "inundation", "zones", "sea_level", "sea_depth", "sea_class"};
static_assert(sizeof(RASTER) / sizeof(RASTER[0]) == MHIP_R_COUNT_, "a name per raster, in the order of mhip_raster");
static_assert(sizeof(PRODUCT) / sizeof(PRODUCT[0]) == HP_COUNT_, "a name per held product, in the order of HeldProduct");

static bool dropped(int written, int product, int variant)
{
    if (held_write_mask(written) & held_made_from(product, variant)) return true;
    for (int p = 0; p < HP_COUNT_; ++p)
        if ((held_goes_with(product) & held_bit(p)) && dropped(written, p, variant)) return true;
    return false;
}

static bool goes_when(int product, int other)      // `other` is dropped, a new call of its entry point included: does `product` go?
{
    for (int p = 0; p < HP_COUNT_; ++p)
        if ((held_goes_with(product) & held_bit(p)) && (p == other || goes_when(p, other))) return true;
    return false;
}

int main()
{
    for (int w = 0; w < MHIP_R_COUNT_; ++w)
        for (int p = 0; p < HP_COUNT_; ++p)
            for (int source : {MHIP_R_FILLED, MHIP_R_DEM})
                for (bool labels : {true, false})
                    std::printf("%s %s %s:%s %s\n", RASTER[w], PRODUCT[p], RASTER[source], labels ? "labels" : "nolabels",
                                dropped(w, p, held_variant(source, labels)) ? "dropped" : "survives");
    for (int p = 0; p < HP_COUNT_; ++p)
        for (int q = 0; q < HP_COUNT_; ++q)
            if (q != p) std::printf("call %s %s %s\n", PRODUCT[p], PRODUCT[q], goes_when(q, p) ? "dropped" : "survives");
    return 0;
}
