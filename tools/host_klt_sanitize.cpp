// host_klt_sanitize.cpp -- stand-alone check of the host layer's additions for hip_klt (include/ofps_hip.h N3) under AddressSanitizer +
// UndefinedBehaviorSanitizer: the record-buffer sizing from ofps_hip_klt_slot_count (ofps::klt_record_floats) and the decoder's properties'
// way -- through ofps::klt_decoder_props, the list HipKltDecoder::props_mut itself returns -- from a saved configuration's JSON through
// transfer_props into a plugin object and back out through props().  No GPU, no context: of the library only its two pure functions
// (ofps_hip_klt_slot_count, ofps_hip_cv_grid) are called.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_klt_sanitize.cpp ofps_amd/host/ofps_host.cpp \
//       -Lofps_amd -lofps_hip -Wl,-rpath,$PWD/ofps_amd -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -o host_klt_sanitize
//   ./host_klt_sanitize                 prints "ok" and exits 0
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../ofps_amd/host/ofps_host.hpp"

using namespace ofps;

namespace {

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the decoder's own property list (ofps::klt_decoder_props, what HipKltDecoder::props_mut returns) over storage that needs no context
struct KltProps : Properties {
    size_t max_w = 150, max_h = 150, levels = 4, radius = 7, iters = 10;
    bool process_fullres = true;
    KltSettings set;
    std::vector<std::pair<std::string, PropertyMut>> props_mut() override {
        return klt_decoder_props({&max_w, &max_h, &process_fullres, &set, &levels, &radius, &iters});
    }
};

bool throws(size_t w, size_t h, size_t max_w, size_t max_h, bool fullres, size_t cell) {
    try { (void)klt_record_floats(w, h, max_w, max_h, fullres, cell); } catch (const Error&) { return true; }
    return false;
}

}  // namespace

int main() {
    // ---- the record buffer: four floats per slot of the cell lattice, partial cells counted
    CHECK(ofps_hip_klt_slot_count(1920, 1080, 16) == 120 * 68 && ofps_hip_klt_slot_count(97, 65, 16) == 35 && ofps_hip_klt_slot_count(97, 65, 12) == 0);
    CHECK(klt_record_floats(1920, 1080, 150, 150, true, 16) == 4 * 120 * 68);
    CHECK(klt_record_floats(3840, 2160, 0, 0, true, 8) == 4 * 480 * 270);            // the cap is not looked at on full-size frames
    CHECK(klt_record_floats(97, 65, 150, 150, true, 32) == 4 * 4 * 3);
    int gw = 0, gh = 0;
    CHECK(ofps_hip_cv_grid(1920, 1080, 150, 150, &gw, &gh) == 0 && gw == 150 && gh == 84);
    CHECK(klt_record_floats(1920, 1080, 150, 150, false, 8) == 4 * 19 * 11);         // the reduced frames' lattice: ceil(150 / 8) x ceil(84 / 8)
    std::vector<float> out(klt_record_floats(1920, 1080, 150, 150, true, 8));
    out.front() = 1.0f; out.back() = 2.0f;                                           // the whole buffer is the vector's
    CHECK(out.size() == 4 * 240 * 135);
    CHECK(throws(1920, 1080, 150, 150, true, 12) && throws(1920, 1080, 150, 150, true, 0) && throws(1920, 1080, 150, 150, true, 33));
    CHECK(throws(1920, 1080, 150, 150, true, (size_t)-1) && throws(0, 1080, 150, 150, true, 16) && throws(1920, (size_t)1 << 40, 150, 150, true, 16));
    CHECK(throws(1920, 1080, 0, 150, false, 16) && throws(1920, 1080, (size_t)1 << 33, 150, false, 16) && !throws(1920, 1080, 0, 0, true, 16));

    // ---- the properties: listed, set, read back, and carried by a saved configuration
    KltProps p;
    size_t listed = 0;
    for (const auto& [name, v] : p.props()) {
        const auto* u = std::get_if<BoundedProp<size_t>>(&v);
        if (name == "Cell size") listed += u && u->val == 16 && u->min == 8 && u->max == 32;
        if (name == "Score radius") listed += u && u->val == 2 && u->min == 1 && u->max == 3;
        if (name == "Min score") listed += u && u->val == 1 && u->min == 1 && u->max == kKltMaxScore;
        if (name == "Min eigenvalue") listed += u && u->val == 1 && u->min == 1 && u->max == kKltMaxEig;
        if (name == "Max residual") listed += u && u->val == 0 && u->min == 0 && u->max == kKltMaxResidual;
        if (name == "Levels") listed += u && u->val == 4 && u->min == 1 && u->max == 6;
        if (name == "Window radius") listed += u && u->val == 7 && u->min == 1 && u->max == 7;
        if (name == "Iterations") listed += u && u->val == 10 && u->min == 1 && u->max == 30;
        if (name == "Mean removal") listed += std::holds_alternative<bool>(v) && !std::get<bool>(v);      // N3m: a boolean, off by default
        if (name == "Consistency check") listed += u && u->val == 0 && u->min == 0 && u->max == 4096;     // N3f: 1/256 pixel, 0 = off
        if (name == "Prediction") listed += std::holds_alternative<bool>(v) && !std::get<bool>(v);         // N3p: a boolean, off by default
    }
    CHECK(listed == 11);
    {
        const auto all = p.props();                          // "Iterations", "Mean removal", "Consistency check", and the extension "Prediction" last
        CHECK(all.size() >= 4 && all[all.size() - 4].first == "Iterations" && all[all.size() - 3].first == "Mean removal");
        CHECK(all[all.size() - 2].first == "Consistency check" && all.back().first == "Prediction");
        CHECK(klt_props({&p.max_w, &p.max_h, &p.process_fullres, &p.set, &p.levels, &p.radius, &p.iters}).back().first == "Consistency check");
    }
    CHECK(p.set_prop("Prediction", Property{true}) && p.set.prediction);
    CHECK(p.set_prop("Prediction", Property{BoundedProp<size_t>{0, 0, 1}}) && p.set.prediction);       // a mismatched kind is ignored
    CHECK(!p.set_prop("Predictions", Property{true}));
    CHECK(p.set_prop("Consistency check", Property{BoundedProp<size_t>{64, 0, kKltMaxFb}}) && p.set.fb_limit == 64);
    CHECK(p.set_prop("Consistency check", Property{true}) && p.set.fb_limit == 64);           // a mismatched kind is ignored
    CHECK(p.set_prop("Mean removal", Property{true}) && p.set.mean_removal);
    CHECK(p.set_prop("Mean removal", Property{BoundedProp<size_t>{0, 0, 1}}) && p.set.mean_removal);    // a mismatched kind is ignored
    CHECK(p.set_prop("Max residual", Property{BoundedProp<size_t>{160, 0, kKltMaxResidual}}) && p.set.max_residual == 160);
    CHECK(p.set_prop("Max residual", Property{true}) && p.set.max_residual == 160);           // a mismatched kind is ignored (properties.rs:180-188)
    CHECK(!p.set_prop("Max residuals", Property{BoundedProp<size_t>{1, 0, kKltMaxResidual}}));
    const std::string cfg = R"({"decoder": [{"selected_plugin": "hip_klt", "arg": "clip.raw?w=64&h=48", "extra": false}, true],
        "detector": [{"selected_plugin": "hip_block_motion", "arg": "", "extra": null}, true],
        "settings": {"worker": {"decoder_properties": {"Cell size": {"Usize": {"val": 8, "min": 8, "max": 32}},
        "Max residual": {"Usize": {"val": 64, "min": 0, "max": 4080}}, "Levels": {"Usize": {"val": 3, "min": 1, "max": 6}},
        "Process Fullres": {"Bool": false}, "Mean removal": {"Bool": true}, "Consistency check": {"Usize": {"val": 16, "min": 0, "max": 4096}},
        "Prediction": {"Bool": true},
        "Not a property of this plugin": {"Bool": true}}, "realtime_processing": false,
        "detector_properties": {}}, "overlay_mf": false, "max_frame_gap": 2, "min_frames": 2,
        "draw_perf_stats": {"summary_window": false, "graph_window": false}}})";
    try {
        const MotionDetectionConfig c = MotionDetectionConfig::from_json(cfg);
        KltProps q;
        transfer_props(c.decoder_properties, q);
        CHECK(q.set.cell == 8 && q.set.max_residual == 64 && q.levels == 3 && !q.process_fullres && q.radius == 7 && q.set.min_eig == 1);
        CHECK(q.set.mean_removal && !KltProps().set.mean_removal);
        CHECK(q.set.fb_limit == 16 && KltProps().set.fb_limit == 0);
        CHECK(q.set.prediction && !KltProps().set.prediction);
        CHECK(klt_record_floats(64, 48, q.max_w, q.max_h, true, q.set.cell) == 4 * 8 * 6);
        size_t seen = 0;
        for (const auto& [name, v] : q.props())
            if (name == "Cell size") seen = std::get<BoundedProp<size_t>>(v).val;
        bool zm = false;
        for (const auto& [name, v] : q.props())
            if (name == "Mean removal") zm = std::get<bool>(v);
        CHECK(zm);
        size_t fb = 0;
        for (const auto& [name, v] : q.props())
            if (name == "Consistency check") fb = std::get<BoundedProp<size_t>>(v).val;
        CHECK(fb == 16);
        CHECK(seen == 8);                                                            // and out again, as a saved configuration would store it
    } catch (const Error& e) {
        std::fprintf(stderr, "configuration: %s\n", e.what());
        ++failures;
    }
    std::puts(failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
