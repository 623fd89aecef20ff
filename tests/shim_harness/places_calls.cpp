// Call lines of the place-recognition part of the C++ shim (include/elimaloc/place_database.hpp: PlaceConfig, PlaceQuery, PlaceDatabase),
// compiled by tests/test_places_abi.py as tests/shim_harness/build_calls.cpp is: the Eigen-typed form against tests/fake_eigen, C++14 and
// C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device.
#include "place_database.hpp"

// two scans described and added, the database saved and loaded into a second one, one scan queried against both: the candidates found
size_t candidates_after_reload(const std::vector<PointStruct>& scan, const Eigen::Matrix4d& level) {
    PlaceConfig config;
    config.n_rings = 8;
    config.r_max_m = 34.0;
    PlaceDatabase places(config, 16), loaded(config, 16);
    const PlaceTables tables = places.Tables();
    const PlaceDatabase::Scans scans(2, scan);
    const PlaceDatabase::Levels levels(2, level);
    std::vector<elm_places_stats> stats;
    const std::vector<uint64_t> described = places.Describe(scans, &levels, &stats);
    const std::vector<elm_places_stats> added = places.Add(scans, std::vector<int64_t>{7, 9}, &levels);
    std::vector<uint64_t> words;
    std::vector<int64_t> ids;
    std::vector<uint32_t> n_bits;
    places.Download(0, places.Size(), words, ids, n_bits);
    loaded.AddDescriptors(words, ids);
    PlaceQuery query;
    query.top_k = 2;
    query.min_dice_q16 = 1000;
    query.exclude_id_lo = query.exclude_id_hi = 9;
    std::vector<elm_place_match> matches;
    const std::vector<std::vector<elm_place_candidate>> by_scan = places.Query(PlaceDatabase::Scans(1, scan), query, nullptr, &matches);
    const std::vector<std::vector<elm_place_candidate>> by_words = loaded.Match(described, query);
    size_t n = tables.dir.size() + stats.size() + added.size() + matches.size() + places.Words();
    for (const std::vector<elm_place_candidate>& c : by_scan) n += c.size();
    for (const std::vector<elm_place_candidate>& c : by_words) n += c.size();
    loaded.Reset();
    return n + loaded.Size();
}

int main(int argc, char**) {
    if (argc > 1) return (int)candidates_after_reload(std::vector<PointStruct>(1), Eigen::Matrix4d::Identity());
    return 0;
}
