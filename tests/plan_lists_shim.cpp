// plan_lists_shim.cpp — test infrastructure: the workgroup lists of a plan, for tests/helpers.py (plan_lists). Compiled by the
// tests with g++ together with heat_amd/csrc/plan.cpp into a temporary directory and loaded with ctypes; not part of the product.
// out [kPlanListsOut] int64: fblocks[c][g2].size() [18 * 4] | team_supers[c].size() [18] | n_stream_tiles[c] [18] | the largest
// FusedBlock::n_zones over all lists | ideal_resident_reason, has_chunks[c] taken from the tiles as batch.hip does | small tiles,
// cavity-free small tiles, streamed small tiles with a cavity (Plan::n_small_tiles, n_small_plain_tiles, n_smallcav_stream_tiles).
#include <string>

#include "../heat_amd/csrc/plan.hpp"

constexpr int kPlanListsOut = heat::kNumFast * 6 + 5;

extern "C" int plan_lists(const heat_batch_desc *desc, const heat_batch_options *opt, int64_t *out, int n_out) {
    if (n_out != kPlanListsOut) return HEAT_E_INVALID_ARG;
    heat::Plan p;
    std::string err;
    const int rc = heat::make_plan(desc, *opt, p, err);
    if (rc) return rc;
    size_t n_blocks[heat::kNumFast][4], n_supers[heat::kNumFast];
    bool has_chunks[heat::kNumFast];
    int64_t most_zones = 0;
    for (int c = 0; c < heat::kNumFast; c++) {
        for (int g2 = 0; g2 < 4; g2++) {
            out[c * 4 + g2] = (int64_t)(n_blocks[c][g2] = p.fblocks[c][g2].size());
            for (const heat::FusedBlock &fb : p.fblocks[c][g2]) most_zones = fb.n_zones > most_zones ? fb.n_zones : most_zones;
        }
        out[heat::kNumFast * 4 + c] = (int64_t)(n_supers[c] = p.team_supers[c].size());
        out[heat::kNumFast * 5 + c] = p.n_stream_tiles[c];
        has_chunks[c] = false;
        for (const heat::FastTile &ft : p.fast_tiles[c]) has_chunks[c] = has_chunks[c] || (ft.k & heat::kTileChunkyBit) != 0;
    }
    int64_t *tail = out + heat::kNumFast * 6;
    tail[0] = most_zones;
    tail[1] = heat::ideal_resident_reason(n_blocks, n_supers, has_chunks);
    tail[2] = p.n_small_tiles, tail[3] = p.n_small_plain_tiles, tail[4] = p.n_smallcav_stream_tiles;
    return HEAT_OK;
}
