// place_database.hpp -- place recognition (include/elimaloc_hip.h, "place recognition"): the C++ face of elm_places in the shim's types.
// A database of binary scan descriptors resident on the device, searched exactly: a query against every entry at every one of the 64
// yaw shifts.  The descriptor, the match and the selection are those of the C header.  Scans are uploaded for the call; a level is the
// scan's levelling pose (sensor roll and pitch, and height), identity when none is given.
#pragma once
#include <vector>

#include "registration.hpp"

struct PlaceConfig {
    int n_rings = 16, n_layers = 8;
    double r_min_m = 2.0, r_max_m = 42.0, z_min_m = -3.0, z_max_m = 9.0;
    elm_places_config c_struct() const {
        elm_places_config c;
        elm_places_config_default(&c);
        c.n_rings = n_rings;
        c.n_layers = n_layers;
        c.r_min_m = r_min_m;
        c.r_max_m = r_max_m;
        c.z_min_m = z_min_m;
        c.z_max_m = z_max_m;
        return c;
    }
};

struct PlaceQuery {
    int top_k = 1;
    uint32_t min_dice_q16 = 0;
    int64_t exclude_id_lo = 0, exclude_id_hi = -1; // lo > hi: nothing is excluded
    elm_places_query_config c_struct() const {
        elm_places_query_config c;
        c.top_k = top_k;
        c.min_dice_q16 = min_dice_q16;
        c.exclude_id_lo = exclude_id_lo;
        c.exclude_id_hi = exclude_id_hi;
        return c;
    }
};

struct PlaceTables {
    std::vector<double> ring_edge2, z_edge, dir; // n_rings + 1, n_layers + 1, 64 x 2
};

class PlaceDatabase {
public:
    using RadarPointVector = VoxelHashMap::RadarPointVector;
    using Scans = std::vector<RadarPointVector>;
    using Levels = std::vector<elimaloc::Matrix4d>;
    explicit PlaceDatabase(const PlaceConfig& config = PlaceConfig(), int capacity = 1024) : cfg_(config.c_struct()) {
        elimaloc::check(elm_places_create(VoxelHashMap::ctx(), &cfg_, capacity, &pl_), VoxelHashMap::ctx(), "elm_places_create");
    }
    PlaceDatabase(const PlaceDatabase&) = delete; // owns device memory
    PlaceDatabase& operator=(const PlaceDatabase&) = delete;
    ~PlaceDatabase() { elm_places_destroy(pl_); }

    inline size_t Words() const { return (size_t)cfg_.n_rings * (size_t)cfg_.n_layers; }
    inline PlaceTables Tables() const {
        PlaceTables t;
        t.ring_edge2.resize((size_t)cfg_.n_rings + 1);
        t.z_edge.resize((size_t)cfg_.n_layers + 1);
        t.dir.resize(2 * ELM_PLACES_SECTORS);
        elimaloc::check(elm_places_tables(&cfg_, t.ring_edge2.data(), t.z_edge.data(), t.dir.data()), VoxelHashMap::ctx(), "elm_places_tables");
        return t;
    }
    inline size_t Size() const {
        size_t n = 0;
        elimaloc::check(elm_places_size(VoxelHashMap::ctx(), pl_, &n), VoxelHashMap::ctx(), "elm_places_size");
        return n;
    }
    inline void Reset() { elimaloc::check(elm_places_reset(VoxelHashMap::ctx(), pl_), VoxelHashMap::ctx(), "elm_places_reset"); }

    // the descriptors of the scans, [scans.size()][Words()]; the database is not touched
    inline std::vector<uint64_t> Describe(const Scans& scans, const Levels* levels = nullptr, std::vector<elm_places_stats>* stats = nullptr) {
        Uploaded up(scans, levels);
        std::vector<uint64_t> words(scans.size() * Words() + 1);
        std::vector<elm_places_stats> st(scans.size() + 1);
        elimaloc::check(elm_places_describe(VoxelHashMap::ctx(), pl_, up.handles.data(), up.levels(), (int)scans.size(), words.data(), st.data()),
                        VoxelHashMap::ctx(), "elm_places_describe");
        words.resize(scans.size() * Words());
        st.resize(scans.size());
        if (stats) *stats = st;
        return words;
    }
    // the same descriptors appended as entries with these ids
    inline std::vector<elm_places_stats> Add(const Scans& scans, const std::vector<int64_t>& ids, const Levels* levels = nullptr) {
        elimaloc::check(ids.size() == scans.size() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(), "PlaceDatabase::Add: one id per scan");
        Uploaded up(scans, levels);
        std::vector<elm_places_stats> st(scans.size() + 1);
        elimaloc::check(elm_places_add(VoxelHashMap::ctx(), pl_, up.handles.data(), up.levels(), ids.data(), (int)scans.size(), st.data()),
                        VoxelHashMap::ctx(), "elm_places_add");
        st.resize(scans.size());
        return st;
    }
    inline void AddDescriptors(const std::vector<uint64_t>& words, const std::vector<int64_t>& ids) {
        elimaloc::check(words.size() == ids.size() * Words() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(),
                        "PlaceDatabase::AddDescriptors: Words() words per id");
        elimaloc::check(elm_places_add_words(VoxelHashMap::ctx(), pl_, words.data(), ids.data(), ids.size()), VoxelHashMap::ctx(),
                        "elm_places_add_words");
    }
    inline void Download(size_t first, size_t count, std::vector<uint64_t>& words, std::vector<int64_t>& ids, std::vector<uint32_t>& n_bits) const {
        words.assign(count * Words() + 1, 0);
        ids.assign(count + 1, 0);
        n_bits.assign(count + 1, 0);
        elimaloc::check(elm_places_download(VoxelHashMap::ctx(), pl_, first, count, words.data(), ids.data(), n_bits.data()), VoxelHashMap::ctx(),
                        "elm_places_download");
        words.resize(count * Words());
        ids.resize(count);
        n_bits.resize(count);
    }
    // per query descriptor (words [n][Words()]) its candidates in rank order; matches, when given: every (query, entry) pair
    inline std::vector<std::vector<elm_place_candidate>> Match(const std::vector<uint64_t>& words, const PlaceQuery& query = PlaceQuery(),
                                                               std::vector<elm_place_match>* matches = nullptr) {
        const size_t n = words.size() / Words();
        Answer a(n, query, matches ? Size() : 0);
        elimaloc::check(elm_places_match_words(VoxelHashMap::ctx(), pl_, words.data(), (int)n, a.cfgs.data(), a.cands.data(), a.counts.data(),
                                               matches ? a.matches.data() : nullptr),
                        VoxelHashMap::ctx(), "elm_places_match_words");
        return a.take(matches);
    }
    // the same on scans: described into scratch, then matched
    inline std::vector<std::vector<elm_place_candidate>> Query(const Scans& scans, const PlaceQuery& query = PlaceQuery(),
                                                               const Levels* levels = nullptr, std::vector<elm_place_match>* matches = nullptr) {
        Uploaded up(scans, levels);
        Answer a(scans.size(), query, matches ? Size() : 0);
        elimaloc::check(elm_places_query(VoxelHashMap::ctx(), pl_, up.handles.data(), up.levels(), (int)scans.size(), a.cfgs.data(), a.cands.data(),
                                         a.counts.data(), matches ? a.matches.data() : nullptr, nullptr),
                        VoxelHashMap::ctx(), "elm_places_query");
        return a.take(matches);
    }

private:
    struct Uploaded { // the scans resident for one call, and their levels as one column-major block
        std::vector<const elm_scan*> handles;
        std::vector<double> block;
        Uploaded(const Scans& scans, const Levels* lv) {
            elimaloc::check(!lv || lv->size() == scans.size() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(), "PlaceDatabase: one level per scan");
            if (lv) {
                for (const elimaloc::Matrix4d& T : *lv) block.insert(block.end(), T.data(), T.data() + 16);
                block.push_back(0.0);
            }
            handles.reserve(scans.size() + 1);
            try {
                for (const RadarPointVector& scan : scans) {
                    std::vector<float> xyz(3 * scan.size() + 3);
                    for (size_t i = 0; i < scan.size(); ++i)
                        for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)scan[i].pose(k);
                    elm_scan* s = nullptr;
                    elimaloc::check(elm_scan_upload(VoxelHashMap::ctx(), xyz.data(), scan.size(), scan.size(), &s), VoxelHashMap::ctx(),
                                    "elm_scan_upload");
                    handles.push_back(s);
                }
            } catch (...) { // the destructor of a half-built object does not run: release what is already up
                release();
                throw;
            }
        }
        Uploaded(const Uploaded&) = delete;
        Uploaded& operator=(const Uploaded&) = delete;
        ~Uploaded() { release(); }
        void release() {
            for (const elm_scan* s : handles) elm_scan_destroy(const_cast<elm_scan*>(s));
            handles.clear();
        }
        const double* levels() const { return block.empty() ? nullptr : block.data(); }
    };
    struct Answer {
        std::vector<elm_places_query_config> cfgs;
        std::vector<elm_place_candidate> cands;
        std::vector<int32_t> counts;
        std::vector<elm_place_match> matches;
        Answer(size_t n, const PlaceQuery& q, size_t size)
            : cfgs(n + 1, q.c_struct()), cands((n + 1) * ELM_PLACES_MAX_TOP_K), counts(n + 1, 0), matches(n * size + 1) {}
        std::vector<std::vector<elm_place_candidate>> take(std::vector<elm_place_match>* m) {
            const size_t n = counts.size() - 1;
            std::vector<std::vector<elm_place_candidate>> out(n);
            for (size_t q = 0; q < n; ++q)
                out[q].assign(cands.begin() + (long)(q * ELM_PLACES_MAX_TOP_K), cands.begin() + (long)(q * ELM_PLACES_MAX_TOP_K) + counts[q]);
            if (m) {
                matches.pop_back();
                *m = matches;
            }
            return out;
        }
    };
    elm_places_config cfg_;
    elm_places* pl_ = nullptr;
};
