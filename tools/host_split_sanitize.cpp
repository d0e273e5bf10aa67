// host_split_sanitize.cpp -- stand-alone check of the host layer's additions for hip_sad's split blocks (include/ofps_hip.h N1s) under
// AddressSanitizer + UndefinedBehaviorSanitizer: the record-buffer arithmetic (ofps::sad_record_floats) and the "Split blocks" property's
// way from a saved configuration's JSON through transfer_props into a plugin object and back out through props().  No GPU, no context: the
// program links the library for ofps_host.cpp's other symbols and never calls into it.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_split_sanitize.cpp ofps_amd/host/ofps_host.cpp \
//       -Lofps_amd -lofps_hip -Wl,-rpath,$PWD/ofps_amd -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -o host_split_sanitize
//   ./host_split_sanitize               prints "ok" and exits 0
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../ofps_amd/host/ofps_host.hpp"

using namespace ofps;

namespace {

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the decoder's property table without its context: the same names, bounds and storage
struct SadProps : Properties {
    size_t block = 16, range = 16, split = 0;
    bool pruned = false, quarter_pel = false;
    std::vector<std::pair<std::string, PropertyMut>> props_mut() override {
        return {{"Block size", PropertyMut::usize(&block, 8, 16)}, {"Search range", PropertyMut::usize(&range, 8, 32)},
                {"Exact pruning", PropertyMut::boolean(&pruned)}, {"Quarter pel", PropertyMut::boolean(&quarter_pel)},
                {"Split blocks", PropertyMut::usize(&split, 0, kSadSplitMax)}};
    }
};

bool throws(size_t records) {
    try { (void)sad_record_floats(records); } catch (const Error&) { return true; }
    return false;
}

}  // namespace

int main() {
    // ---- the record buffer: capacity records of four floats
    CHECK(sad_record_floats(0) == 0);
    const size_t nblk_1080p = (1920 / 16) * (1080 / 16), nblk_4k = (3840 / 8) * (2160 / 8);
    CHECK(sad_record_floats(nblk_1080p) == 4 * nblk_1080p && sad_record_floats(4 * nblk_1080p) == 16 * nblk_1080p);
    CHECK(sad_record_floats(4 * nblk_4k) == 16 * nblk_4k);
    std::vector<float> out(sad_record_floats(4 * nblk_1080p));
    out.front() = 1.0f; out.back() = 2.0f;                              // the whole buffer is the vector's
    CHECK(out.size() == 16 * nblk_1080p);
    CHECK(throws(std::numeric_limits<size_t>::max()) && throws(std::numeric_limits<size_t>::max() / 4 + 1));
    CHECK(throws(std::vector<float>().max_size() / 4 + 1) && !throws(1u << 20));

    // ---- the property: listed, set, read back, and carried by a saved configuration
    SadProps p;
    bool listed = false;
    for (const auto& [name, v] : p.props())
        if (name == "Split blocks") {
            const auto* u = std::get_if<BoundedProp<size_t>>(&v);
            listed = u && u->val == 0 && u->min == 0 && u->max == kSadSplitMax;
        }
    CHECK(listed);
    CHECK(p.set_prop("Split blocks", Property{BoundedProp<size_t>{16, 0, kSadSplitMax}}) && p.split == 16);
    CHECK(p.set_prop("Split blocks", Property{true}) && p.split == 16);         // a mismatched kind is ignored (properties.rs:180-188)
    CHECK(!p.set_prop("Split block", Property{BoundedProp<size_t>{1, 0, kSadSplitMax}}));
    const std::string cfg = R"({"decoder": [{"selected_plugin": "hip_sad", "arg": "clip.raw?w=64&h=48", "extra": false}, true],
        "detector": [{"selected_plugin": "hip_block_motion", "arg": "", "extra": null}, true],
        "settings": {"worker": {"decoder_properties": {"Split blocks": {"Usize": {"val": 32, "min": 0, "max": 4080}},
        "Quarter pel": {"Bool": false}, "Not a property of this plugin": {"Bool": true}}, "realtime_processing": false,
        "detector_properties": {}}, "overlay_mf": false, "max_frame_gap": 2, "min_frames": 2,
        "draw_perf_stats": {"summary_window": false, "graph_window": false}}})";
    try {
        const MotionDetectionConfig c = MotionDetectionConfig::from_json(cfg);
        SadProps q;
        transfer_props(c.decoder_properties, q);
        CHECK(q.split == 32 && !q.quarter_pel && q.block == 16);
        size_t seen = 0;
        for (const auto& [name, v] : q.props())
            if (name == "Split blocks") seen = std::get<BoundedProp<size_t>>(v).val;
        CHECK(seen == 32);                                                      // and out again, as a saved configuration would store it
    } catch (const Error& e) {
        std::fprintf(stderr, "configuration: %s\n", e.what());
        ++failures;
    }
    std::puts(failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
