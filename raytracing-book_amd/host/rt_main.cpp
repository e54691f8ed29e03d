// rt_main.cpp — `rtrender`, the command-line front end of the reference
// (src/main/java/net/bowen/Main.java:6-70) over the rt.h / rt_scene.h C ABIs.
//
// Same options, defaults and error behaviour as the reference's commons-cli
// parser:
//   -h,--help  -s,--scene <id>=0  -r,--resolution <W:H>=500:300
//   -spp,--sample-per-pixel <n>=20  -md,--max-depth <n>=5  -o,--output <png>
// A parse error prints the parser message and the help text and exits 1
// (Main.java:16-20); a non-integer value exits 1 with the message of the
// NumberFormatException Integer.parseInt throws; an unknown scene id exits 1
// with "Invalid scene ID: <id>" (Scene.java:29).
//
// Where the reference opens a window and dispatches one frame per vsync until
// samplePerPixel frames are done (Window.java:250-281, RaytraceExecutor.java:
// 100-156), rtrender queues the frames in batches of --frames-per-launch on the
// MI355X (rt_render), then runs the completion listeners of Window.java:213-233:
// "All samples have completed in ..." and, with -o, Texture.saveAsPNG.
//
// MI355X-only options (no reference counterpart): --seed (scene + per-frame
// factor seed; the reference uses the unseeded Math.random), --devices
// (comma-separated HIP device ids, rows striped across them), --frames-per-launch.
//
// Progressive preview, the headless form of the window loop
// (Window.java:250-281): --preview <png> rewrites that PNG with the running mean
// every --preview-every frames (drawResult: the image so far, through
// Texture.saveAsPNG) and prints GuiRenderer.draw's status lines
// (GuiRenderer.java:48-62): "Last raytrace took: <ms> ms." and
// "Sample: <n>/<spp>." (+ "Render completed in: ..." once complete).
//
// Noise target: --noise <x> renders batches of --frames-per-launch frames until the image's
// estimated relative noise (rt_render_until: per-pixel sample moments, rt.h) is at most x, with
// -spp as the cap, and prints "Noise target: <frames> frames, noise <value> (...)".  One device.
// With --adaptive the target holds per 8x8 tile (rt_render_adaptive): a tile stops once it has
// --min-frames frames (default 16) and its own estimate is within the target, the others go on; it
// prints "Adaptive: <max frames> frames, <samples> of <W*H*max frames> samples, noise <value> (...)".
//
// Preview filter: --denoise turns the sample moments on (the image's bits do not change) and passes the
// image through rt_denoise (the variance-guided a-trous filter of rt.h; --denoise-levels, --denoise-k)
// before it is saved: -o receives the filtered image, and so does every --preview update once two
// frames exist; --raw-output <png> also saves the image as rendered.  One device; works with --noise
// and --adaptive.
//
// A moving camera: --moves <K> --move-shift <S> --move-frames <N> turns the sample moments and the history
// variance on and, after the normal render, takes the camera through K poses, each S viewport widths along
// pixel_delta_u from the one before (camera_pos and up_left shifted by the same vector), with N frames per
// pose through rt_render_moved: history kept, the new view rendered, reprojected, filtered and presented on
// the device.  Each pose's frame (rt_read_presented, alpha dropped) is saved as <output stem>.moveNN.png.
// The frames of pose k (1-based) take the factors of frame indices spp + (k - 1) * N onwards.  One device; needs -o.
// --move-refine <K> spends K more frames per pose on the 8x8 tiles the history does not reach
// (rt_render_moved_refined); --move-refine-count <C> names the count below which a pixel is short (default
// N + K) and --move-refine-tiles <M> caps the tiles refined per pose.  Pose k then takes the factors of frame
// indices spp + (k - 1) * (N + K) onwards, N for the pose and K for the refinement.
// --move-noise <x> renders each pose until every 8x8 tile meets the relative noise x or a round cap
// (rt_render_moved_to_noise): --move-noise-batch <B> frames per round (default 1), --move-noise-rounds <R> rounds at
// most (default 4), --move-noise-count <C> the count below which a pixel is thin (default 2).  Pose k then takes the
// factors of frame indices spp + (k - 1) * (N + B * R) onwards.  It does not combine with --move-refine.
// --move-misses reprojects the pixels whose centre ray hits nothing by the ray's direction too
// (rt_set_reproject_misses): the background keeps its history, and fewer tiles qualify for --move-refine.
#include "rt/rt.h"
#include "rt/rt_scene.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <limits.h>
#include <stdlib.h>

namespace {

struct Opt {
    const char* shrt;
    const char* lng;
    bool has_arg;
    const char* desc;
};

// commons-cli Options in Main.getOptions order (Main.java:43-70)
enum { O_HELP, O_SCENE, O_RES, O_SPP, O_DEPTH, O_OUT, O_SEED, O_DEVICES, O_PER_LAUNCH, O_PREVIEW, O_PREVIEW_EVERY, O_NOISE, O_ADAPTIVE, O_MIN_FRAMES, O_DENOISE, O_DENOISE_LEVELS, O_DENOISE_K, O_RAW_OUT, O_DENOISE_GUIDES, O_DENOISE_KN, O_DENOISE_KZ, O_DENOISE_KA, O_FEATURES_OUT, O_MOVES, O_MOVE_SHIFT, O_MOVE_FRAMES, O_MOVE_REFINE, O_MOVE_REFINE_COUNT, O_MOVE_REFINE_TILES, O_MOVE_MISSES, O_MOVE_NOISE, O_MOVE_NOISE_BATCH, O_MOVE_NOISE_ROUNDS, O_MOVE_NOISE_COUNT, O_N };
const Opt kOpts[O_N] = {
    {"h", "help", false, "print help message"},
    {"s", "scene", true, "scene ID"},
    {"r", "resolution", true, "screen resolution"},
    {"spp", "sample-per-pixel", true, "sample per pixel"},
    {"md", "max-depth", true, "max depth"},
    {"o", "output", true, "output file (must be a .png file)"},
    // MI355X extensions
    {nullptr, "seed", true, "scene and frame RNG seed (default 1)"},
    {nullptr, "devices", true, "comma-separated HIP device ids (default 0)"},
    {nullptr, "frames-per-launch", true, "frames per kernel launch (default 64)"},
    {nullptr, "preview", true, "progressive preview PNG, rewritten every --preview-every frames"},
    {nullptr, "preview-every", true, "frames between preview updates (default: --frames-per-launch)"},
    {nullptr, "noise", true, "stop once the estimated relative noise is at most this (-spp is the cap)"},
    {nullptr, "adaptive", false, "with --noise: stop sampling each 8x8 tile once it meets the target"},
    {nullptr, "min-frames", true, "with --adaptive: frames every tile gets before it may stop (default 16)"},
    {nullptr, "denoise", false, "save the image through the variance-guided preview filter (needs 2 frames)"},
    {nullptr, "denoise-levels", true, "with --denoise: filter levels, 1..5 (default 3)"},
    {nullptr, "denoise-k", true, "with --denoise: edge-stopping width in standard deviations (default 3)"},
    {nullptr, "raw-output", true, "with --denoise: also save the unfiltered image to this .png file"},
    {nullptr, "denoise-guides", false, "with --denoise: guide the filter by first-hit normal, depth and albedo"},
    {nullptr, "denoise-kn", true, "with --denoise-guides: strength of the normal term, >= 0"},
    {nullptr, "denoise-kz", true, "with --denoise-guides: strength of the depth term, >= 0"},
    {nullptr, "denoise-ka", true, "with --denoise-guides: strength of the albedo term, >= 0"},
    {nullptr, "features-output", true, "save first-hit <arg>_normal.png, <arg>_albedo.png and <arg>_depth.png"},
    {nullptr, "moves", true, "after the render: this many camera poses, each saved as <output stem>.moveNN.png"},
    {nullptr, "move-shift", true, "with --moves: viewport widths each pose moves sideways from the one before"},
    {nullptr, "move-frames", true, "with --moves: frames rendered at each pose (reprojected, filtered, presented)"},
    {nullptr, "move-refine", true, "with --moves: extra frames per pose on the 8x8 tiles the history does not reach"},
    {nullptr, "move-refine-count", true, "with --move-refine: a pixel is short below this count (default: the frames a refined tile gets)"},
    {nullptr, "move-refine-tiles", true, "with --move-refine: at most this many tiles refined per pose (default: no cap)"},
    {nullptr, "move-misses", false, "with --moves: reproject the background (pixels that hit nothing) by ray direction too"},
    {nullptr, "move-noise", true, "with --moves: render each pose until every 8x8 tile meets this relative noise"},
    {nullptr, "move-noise-batch", true, "with --move-noise: frames per round on the tiles still above the target (default 1)"},
    {nullptr, "move-noise-rounds", true, "with --move-noise: rounds per pose at most (default 4)"},
    {nullptr, "move-noise-count", true, "with --move-noise: a pixel is thin below this count (default 2)"},
};

// HelpFormatter.printHelp("OpenGL Ray Tracer", options): options sorted by key.
void print_help() {
    std::vector<std::string> left(O_N);
    size_t width = 0;
    for (int i = 0; i < O_N; i++) {
        std::string l = " ";
        l += kOpts[i].shrt ? std::string("-") + kOpts[i].shrt + "," : std::string("   ");
        l += std::string("--") + kOpts[i].lng;
        if (kOpts[i].has_arg) l += " <arg>";
        left[i] = l;
        width = std::max(width, l.size());
    }
    std::vector<int> order(O_N);
    for (int i = 0; i < O_N; i++) order[i] = i;
    auto key = [](int i) { return std::string(kOpts[i].shrt ? kOpts[i].shrt : kOpts[i].lng); };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
    std::printf("usage: OpenGL Ray Tracer\n");
    for (int i : order) std::printf("%-*s   %s\n", (int)width, left[i].c_str(), kOpts[i].desc);
}

[[noreturn]] void parse_fail(const std::string& msg) {
    std::printf("%s\n", msg.c_str());
    print_help();
    std::exit(1);
}

// The reference reports these as uncaught Java exceptions (exit status 1).
[[noreturn]] void uncaught(const char* cls, const std::string& msg) {
    std::fprintf(stderr, "Exception in thread \"main\" %s: %s\n", cls, msg.c_str());
    std::exit(1);
}

// Integer.parseInt: optional sign, decimal digits, 32-bit range.
int parse_int(const std::string& s) {
    bool ok = !s.empty();
    size_t i = (ok && (s[0] == '-' || s[0] == '+')) ? 1 : 0;
    if (i == s.size()) ok = false;
    long long v = 0;
    for (size_t k = i; ok && k < s.size(); k++) {
        if (s[k] < '0' || s[k] > '9') ok = false;
        else if ((v = v * 10 + (s[k] - '0')) > (long long)INT_MAX + 1) ok = false;
    }
    if (ok && s[0] == '-') v = -v;
    if (!ok || v > INT_MAX || v < INT_MIN) uncaught("java.lang.NumberFormatException", "For input string: \"" + s + "\"");
    return (int)v;
}

// RaytraceExecutor.getFinishTimeString (RaytraceExecutor.java:76-89)
std::string finish_time_string(int finish_ms) {
    long long ms = finish_ms;
    long long hours = ms / 3600000, minutes = (ms / 60000) % 60, seconds = (ms / 1000) % 60;
    std::string s;
    if (hours > 0) s += std::to_string(hours) + "hour ";
    if (minutes > 0) s += std::to_string(minutes) + "minutes ";
    s += std::to_string(seconds) + "." + std::to_string(finish_ms % 1000) + "seconds";
    return s;
}

[[noreturn]] void die(const char* what, const char* msg) {
    std::fprintf(stderr, "%s: %s\n", what, msg ? msg : "");
    std::exit(1);
}

}  // namespace

int main(int argc, char** argv) {
    // commons-cli DefaultParser: "-x v", "-xv" (value attached to a short
    // option), "--long v", "--long=v"; an unknown "-..." token is an error.
    std::string val[O_N];
    bool seen[O_N] = {};
    for (int i = 1; i < argc; i++) {
        std::string t = argv[i];
        if (t.size() < 2 || t[0] != '-') continue;   // stray arguments land in cmd.getArgs()
        int hit = -1;
        std::string attached;
        bool has_attached = false;
        if (t.rfind("--", 0) == 0) {
            std::string name = t.substr(2);
            size_t eq = name.find('=');
            if (eq != std::string::npos) {
                attached = name.substr(eq + 1);
                has_attached = true;
                name = name.substr(0, eq);
            }
            for (int k = 0; k < O_N; k++)
                if (name == kOpts[k].lng) hit = k;
        } else {
            std::string name = t.substr(1);
            for (int k = 0; k < O_N; k++)
                if (kOpts[k].shrt && name == kOpts[k].shrt) hit = k;
            if (hit < 0)   // "-s8": the longest value-taking short option that prefixes the token
                for (int k = 0; k < O_N; k++)
                    if (kOpts[k].shrt && kOpts[k].has_arg && name.rfind(kOpts[k].shrt, 0) == 0 &&
                        (hit < 0 || std::strlen(kOpts[k].shrt) > std::strlen(kOpts[hit].shrt))) {
                        hit = k;
                        attached = name.substr(std::strlen(kOpts[k].shrt));
                        has_attached = true;
                    }
        }
        if (hit < 0) parse_fail("Unrecognized option: " + t);
        seen[hit] = true;
        if (!kOpts[hit].has_arg) continue;
        if (has_attached) {
            val[hit] = attached;
        } else if (i + 1 < argc && !(argv[i + 1][0] == '-' && argv[i + 1][1] != '\0')) {
            val[hit] = argv[++i];
        } else {
            parse_fail(std::string("Missing argument for option: ") + (kOpts[hit].shrt ? kOpts[hit].shrt : kOpts[hit].lng));
        }
    }
    if (seen[O_HELP]) {
        print_help();
        return 0;
    }
    auto get = [&](int k, const char* def) { return seen[k] ? val[k] : std::string(def ? def : ""); };

    // Main.java:30-38
    std::string res = get(O_RES, "500:300");
    size_t colon = res.find(':');
    int width = parse_int(res.substr(0, colon));
    if (colon == std::string::npos)
        uncaught("java.lang.ArrayIndexOutOfBoundsException", "Index 1 out of bounds for length 1");
    size_t colon2 = res.find(':', colon + 1);
    int height = parse_int(res.substr(colon + 1, colon2 == std::string::npos ? std::string::npos : colon2 - colon - 1));
    int scene_id = parse_int(get(O_SCENE, "0"));
    int spp = parse_int(get(O_SPP, "20"));
    int max_depth = parse_int(get(O_DEPTH, "5"));
    std::string output = get(O_OUT, nullptr);
    long long seed = parse_int(get(O_SEED, "1"));
    int per_launch = parse_int(get(O_PER_LAUNCH, "64"));
    std::vector<int> devices;
    {
        std::string d = get(O_DEVICES, "0");
        size_t p = 0;
        while (p <= d.size()) {
            size_t q = d.find(',', p);
            if (q == std::string::npos) q = d.size();
            devices.push_back(parse_int(d.substr(p, q - p)));
            p = q + 1;
        }
    }
    // Scene.java:19-30; scene 9 is the build's Book-1 three-sphere scene
    if (scene_id < 0 || scene_id > 9)
        uncaught("java.lang.IllegalArgumentException", "Invalid scene ID: " + std::to_string(scene_id));
    if (width <= 0 || height <= 0) die("rtrender", "resolution must be positive");
    if (per_launch <= 0) die("rtrender", "--frames-per-launch must be positive");
    const std::string preview = get(O_PREVIEW, nullptr);
    const int preview_every = seen[O_PREVIEW_EVERY] ? parse_int(val[O_PREVIEW_EVERY]) : per_launch;
    if (preview_every <= 0) die("rtrender", "--preview-every must be positive");
    float noise_target = -1.0f;
    if (seen[O_NOISE]) {
        char* end = nullptr;
        noise_target = std::strtof(val[O_NOISE].c_str(), &end);
        if (val[O_NOISE].empty() || *end != '\0' || !(noise_target >= 0.0f))
            die("rtrender", "--noise must be a number >= 0");
        if (devices.size() > 1) die("rtrender", "--noise renders on one device (--devices names more)");
        if (!preview.empty()) die("rtrender", "--noise and --preview do not combine");
        if (spp <= 0) die("rtrender", "--noise needs -spp >= 1 (the cap)");
    }
    if (seen[O_ADAPTIVE] && !seen[O_NOISE]) die("rtrender", "--adaptive needs --noise <x> (the target)");
    if (seen[O_MIN_FRAMES] && !seen[O_ADAPTIVE]) die("rtrender", "--min-frames goes with --adaptive");
    const int min_frames = seen[O_MIN_FRAMES] ? parse_int(val[O_MIN_FRAMES]) : 16;
    if (min_frames < 2) die("rtrender", "--min-frames must be at least 2");
    const bool denoise = seen[O_DENOISE];
    rt_denoise_params dn_params;
    std::memset(&dn_params, 0, sizeof(dn_params));
    dn_params.levels = 3;
    dn_params.k = 3.0f;
    const std::string raw_output = get(O_RAW_OUT, nullptr);
    if (!denoise && (seen[O_DENOISE_LEVELS] || seen[O_DENOISE_K] || seen[O_RAW_OUT]))
        die("rtrender", "--denoise-levels, --denoise-k and --raw-output go with --denoise");
    if (denoise) {
        if (seen[O_DENOISE_LEVELS]) dn_params.levels = parse_int(val[O_DENOISE_LEVELS]);
        if (dn_params.levels < 1 || dn_params.levels > RT_DENOISE_MAX_LEVELS) die("rtrender", "--denoise-levels must be 1..5");
        if (seen[O_DENOISE_K]) {
            char* end = nullptr;
            dn_params.k = std::strtof(val[O_DENOISE_K].c_str(), &end);
            if (val[O_DENOISE_K].empty() || *end != '\0' || !(dn_params.k > 0.0f) || !(dn_params.k <= 3.0e38f))
                die("rtrender", "--denoise-k must be a finite number > 0");
        }
        if (devices.size() > 1) die("rtrender", "--denoise renders on one device (--devices names more)");
        if (spp < 2) die("rtrender", "--denoise needs -spp >= 2 (a variance takes two frames)");
    }
    const bool guides = seen[O_DENOISE_GUIDES];
    if (guides && !denoise) die("rtrender", "--denoise-guides goes with --denoise");
    if (!guides && (seen[O_DENOISE_KN] || seen[O_DENOISE_KZ] || seen[O_DENOISE_KA]))
        die("rtrender", "--denoise-kn, --denoise-kz and --denoise-ka go with --denoise-guides");
    rt_guide_params guide_params;
    std::memset(&guide_params, 0, sizeof(guide_params));
    guide_params.kn = RT_GUIDE_DEFAULT_KN;
    guide_params.kz = RT_GUIDE_DEFAULT_KZ;
    guide_params.ka = RT_GUIDE_DEFAULT_KA;
    {
        const int which[3] = {O_DENOISE_KN, O_DENOISE_KZ, O_DENOISE_KA};
        float* into[3] = {&guide_params.kn, &guide_params.kz, &guide_params.ka};
        for (int i = 0; i < 3; i++) {
            if (!seen[which[i]]) continue;
            char* end = nullptr;
            const float v = std::strtof(val[which[i]].c_str(), &end);
            if (val[which[i]].empty() || *end != '\0' || !(v >= 0.0f) || !(v <= 3.0e38f))
                die("rtrender", (std::string("--") + kOpts[which[i]].lng + " must be a finite number >= 0").c_str());
            *into[i] = v;
        }
    }
    const std::string features_output = get(O_FEATURES_OUT, nullptr);
    if (seen[O_FEATURES_OUT] && features_output.empty()) die("rtrender", "--features-output needs a file prefix");
    if (seen[O_FEATURES_OUT] && devices.size() > 1)
        die("rtrender", "--features-output renders on one device (--devices names more)");

    const bool moving = seen[O_MOVES];
    int moves = 0, move_frames = 0, move_refine = 0, move_refine_tiles = 0;
    float move_shift = 0.0f, move_refine_count = 0.0f;
    if (!moving && (seen[O_MOVE_SHIFT] || seen[O_MOVE_FRAMES])) die("rtrender", "--move-shift and --move-frames go with --moves");
    if (!moving && (seen[O_MOVE_REFINE] || seen[O_MOVE_REFINE_COUNT] || seen[O_MOVE_REFINE_TILES]))
        die("rtrender", "--move-refine, --move-refine-count and --move-refine-tiles go with --moves");
    if (!moving && seen[O_MOVE_MISSES]) die("rtrender", "--move-misses goes with --moves");
    if (!seen[O_MOVE_REFINE] && (seen[O_MOVE_REFINE_COUNT] || seen[O_MOVE_REFINE_TILES]))
        die("rtrender", "--move-refine-count and --move-refine-tiles go with --move-refine");
    const bool noise_moves = seen[O_MOVE_NOISE];
    int move_noise_batch = 1, move_noise_rounds = 4;
    float move_noise = 0.0f, move_noise_count = 0.0f;
    if (!moving && (noise_moves || seen[O_MOVE_NOISE_BATCH] || seen[O_MOVE_NOISE_ROUNDS] || seen[O_MOVE_NOISE_COUNT]))
        die("rtrender", "--move-noise, --move-noise-batch, --move-noise-rounds and --move-noise-count go with --moves");
    if (!noise_moves && (seen[O_MOVE_NOISE_BATCH] || seen[O_MOVE_NOISE_ROUNDS] || seen[O_MOVE_NOISE_COUNT]))
        die("rtrender", "--move-noise-batch, --move-noise-rounds and --move-noise-count go with --move-noise");
    if (noise_moves && seen[O_MOVE_REFINE]) die("rtrender", "--move-noise and --move-refine do not combine");
    if (moving) {
        if (!seen[O_MOVE_SHIFT] || !seen[O_MOVE_FRAMES])
            die("rtrender", "--moves needs --move-shift <S> and --move-frames <N>");
        moves = parse_int(val[O_MOVES]);
        move_frames = parse_int(val[O_MOVE_FRAMES]);
        if (moves < 1) die("rtrender", "--moves must be at least 1");
        if (move_frames < 1) die("rtrender", "--move-frames must be at least 1");
        char* end = nullptr;
        move_shift = std::strtof(val[O_MOVE_SHIFT].c_str(), &end);
        if (val[O_MOVE_SHIFT].empty() || *end != '\0' || !(move_shift >= -3.0e38f && move_shift <= 3.0e38f))
            die("rtrender", "--move-shift must be a finite number");
        if (devices.size() > 1) die("rtrender", "--moves renders on one device (--devices names more)");
        if (output.empty()) die("rtrender", "--moves needs -o <png> (the poses are saved beside it)");
        if (seen[O_MOVE_REFINE]) {
            move_refine = parse_int(val[O_MOVE_REFINE]);
            if (move_refine < 1) die("rtrender", "--move-refine must be at least 1");
            if (move_refine > INT_MAX - move_frames) die("rtrender", "--move-refine is too large");
        }
        if (seen[O_MOVE_REFINE_COUNT]) {
            move_refine_count = std::strtof(val[O_MOVE_REFINE_COUNT].c_str(), &end);
            if (val[O_MOVE_REFINE_COUNT].empty() || *end != '\0' || !(move_refine_count > 0.0f) || !(move_refine_count <= 3.0e38f))
                die("rtrender", "--move-refine-count must be a finite number > 0");
        }
        if (seen[O_MOVE_REFINE_TILES]) {
            move_refine_tiles = parse_int(val[O_MOVE_REFINE_TILES]);
            if (move_refine_tiles < 1) die("rtrender", "--move-refine-tiles must be at least 1");
        }
        if (noise_moves) {
            move_noise = std::strtof(val[O_MOVE_NOISE].c_str(), &end);
            if (val[O_MOVE_NOISE].empty() || *end != '\0' || !(move_noise >= 0.0f) || !(move_noise <= 3.0e38f))
                die("rtrender", "--move-noise must be a finite number >= 0");
            if (seen[O_MOVE_NOISE_BATCH]) move_noise_batch = parse_int(val[O_MOVE_NOISE_BATCH]);
            if (move_noise_batch < 1) die("rtrender", "--move-noise-batch must be at least 1");
            if (seen[O_MOVE_NOISE_ROUNDS]) move_noise_rounds = parse_int(val[O_MOVE_NOISE_ROUNDS]);
            if (move_noise_rounds < 0) die("rtrender", "--move-noise-rounds must be at least 0");
            if ((long long)move_noise_batch * move_noise_rounds > (long long)INT_MAX - move_frames)
                die("rtrender", "--move-noise-batch times --move-noise-rounds is too large");
            if (seen[O_MOVE_NOISE_COUNT]) {
                move_noise_count = std::strtof(val[O_MOVE_NOISE_COUNT].c_str(), &end);
                if (val[O_MOVE_NOISE_COUNT].empty() || *end != '\0' || !(move_noise_count > 0.0f) || !(move_noise_count <= 3.0e38f))
                    die("rtrender", "--move-noise-count must be a finite number > 0");
            }
        }
    }

    rts_scene* scene = nullptr;
    if (rts_build(scene_id, width, height, (uint64_t)seed, nullptr, &scene) != 0) die("rts_build", rts_last_error());
    rts_info info;
    rts_get_info(scene, &info);

    rt_ctx* ctx = nullptr;
    if (rt_create((int)devices.size(), devices.data(), &ctx) != 0) die("rt_create", rt_last_error(nullptr));
    auto chk = [&](int rc, const char* what) {
        if (rc != 0) die(what, rt_last_error(ctx));
    };
    // RaytraceModel.putModelsToProgram, Texture.putData, Camera.init
    for (int b = 0; b < 6; b++) {
        const void* p = nullptr;
        size_t n = 0;
        rts_get_buffer(scene, b, &p, &n);
        chk(rt_upload_buffer(ctx, b, p, n), "rt_upload_buffer");
    }
    for (int s = 0; s < info.n_textures; s++) {
        int fmt = 0, w = 0, h = 0;
        const void* p = nullptr;
        size_t n = 0;
        rts_get_texture(scene, s, &fmt, &w, &h, &p, &n);
        chk(rt_upload_texture(ctx, s, fmt, w, h, p), "rt_upload_texture");
    }
    float ubo[28];
    rts_get_camera(scene, ubo);
    chk(rt_set_camera(ctx, ubo), "rt_set_camera");
    float sqrt_spp, recip;
    rts_spp_uniforms(spp, &sqrt_spp, &recip);   // RaytraceExecutor.setSamplePerPixel
    chk(rt_set_params(ctx, max_depth, info.background, sqrt_spp, recip), "rt_set_params");
    chk(rt_resize(ctx, width, height), "rt_resize");
    if (denoise || moving) chk(rt_set_moments(ctx, 1), "rt_set_moments");
    if (moving) chk(rt_set_history_variance(ctx, 1), "rt_set_history_variance");
    if (seen[O_MOVE_MISSES]) chk(rt_set_reproject_misses(ctx, 1), "rt_set_reproject_misses");
    // the first-hit pass, once: the scene and the camera do not change from here on
    // (with --moves the scene and the first pose's camera: rt_render_moved renders each later pose's)
    if (guides || !features_output.empty() || moving) chk(rt_render_features(ctx), "rt_render_features");
    // the image to save: through the filter with --denoise (once every tile holds two frames), else as rendered
    auto read_shown = [&](float* px, bool filtered) {
        if (filtered && guides) {
            chk(rt_denoise_guided(ctx, &dn_params, &guide_params), "rt_denoise_guided");
            chk(rt_read_denoised(ctx, px), "rt_read_denoised");
        } else if (filtered) {
            chk(rt_denoise(ctx, &dn_params), "rt_denoise");
            chk(rt_read_denoised(ctx, px), "rt_read_denoised");
        } else {
            chk(rt_read_image(ctx, px), "rt_read_image");
        }
    };

    // RaytraceExecutor.raytrace x samplePerPixel, batched per launch
    auto t0 = std::chrono::steady_clock::now();
    std::vector<float> rf((size_t)per_launch);
    uint64_t device_ns = 0;
    std::vector<float> rgba;
    if (seen[O_NOISE]) {
        rt_noise_stats st;
        int frames = 0;
        chk(rt_set_moments(ctx, 1), "rt_set_moments");
        if (seen[O_ADAPTIVE]) {
            chk(rt_render_adaptive(ctx, 1, spp, per_launch, min_frames, (uint64_t)seed, noise_target, &frames, &st),
                "rt_render_adaptive");
            // the samples taken: per tile its pixels x the frames it holds
            int n_tiles = 0;
            chk(rt_read_tile_frames(ctx, nullptr, 0, &n_tiles), "rt_read_tile_frames");
            std::vector<int32_t> counts((size_t)n_tiles);
            chk(rt_read_tile_frames(ctx, counts.data(), n_tiles, &n_tiles), "rt_read_tile_frames");
            const int tiles_x = (width + 7) / 8;
            long long samples = 0;
            for (int t = 0; t < n_tiles; t++)
                samples += (long long)std::min(8, width - (t % tiles_x) * 8) * std::min(8, height - (t / tiles_x) * 8) *
                           counts[(size_t)t];
            std::printf("Adaptive: %d frames, %lld of %lld samples, noise %.6g (%s)\n", frames, samples,
                        (long long)width * height * frames, st.noise, st.converged ? "converged" : "sample cap reached");
        } else {
            chk(rt_render_until(ctx, 1, spp, per_launch, (uint64_t)seed, noise_target, &frames, &st), "rt_render_until");
            std::printf("Noise target: %d frames, noise %.6g (%s)\n", frames, st.noise,
                        st.converged ? "converged" : "sample cap reached");
        }
        spp = frames;
    }
    for (int f0 = seen[O_NOISE] ? spp : 0; f0 < spp;) {
        int n = std::min(per_launch, spp - f0);
        if (!preview.empty()) n = std::min(n, preview_every - f0 % preview_every);   // stop at the next preview
        for (int i = 0; i < n; i++) rf[i] = rt_frame_rand_factor((uint64_t)seed, (uint64_t)(f0 + i));
        chk(rt_render(ctx, f0 + 1, n, rf.data()), "rt_render");
        chk(rt_sync(ctx), "rt_sync");
        uint64_t ns = 0;
        chk(rt_last_render_ns(ctx, &ns), "rt_last_render_ns");
        device_ns += ns;
        f0 += n;
        if (!preview.empty() && (f0 % preview_every == 0 || f0 == spp)) {
            // one pass of the window loop: drawResult + GuiRenderer.draw
            rgba.resize((size_t)width * height * 4);
            read_shown(rgba.data(), denoise && f0 >= 2);
            if (rts_save_png(rgba.data(), width, height, preview.c_str()) != 0)
                uncaught("java.lang.RuntimeException", "Failed to save texture as PNG");
            std::printf("Last raytrace took: %d ms.\n", (int)(ns / 1000000));
            std::printf("Sample: %d/%d.", f0, spp);
            if (f0 == spp) {
                const int ms = (int)std::chrono::duration_cast<std::chrono::milliseconds>(
                                   std::chrono::steady_clock::now() - t0).count();
                std::printf("Render completed in: %s.", finish_time_string(ms).c_str());
            }
            std::printf("\n");
            std::fflush(stdout);
        }
    }
    int finish_ms = (int)std::chrono::duration_cast<std::chrono::milliseconds>(
                        std::chrono::steady_clock::now() - t0).count();
    std::printf("All samples have completed in %s.\n", finish_time_string(finish_ms).c_str());
    if (device_ns > 0)
        std::printf("device time %.3f ms, %.1f Msamples/s (scene %d, %dx%d, %d spp, max_depth %d, %zu device(s))\n",
                    device_ns * 1e-6, (double)width * height * spp / (device_ns * 1e-9) * 1e-6, scene_id, width,
                    height, spp, max_depth, devices.size());

    if (!output.empty()) {   // Window.saveImage (Window.java:227-233)
        std::printf("Saving the result to %s...\n", output.c_str());
        std::vector<float> rgba((size_t)width * height * 4);
        read_shown(rgba.data(), denoise);
        if (denoise) std::printf("Denoise: levels %d, k %g\n", dn_params.levels, (double)dn_params.k);
        if (guides)
            std::printf("Denoise guides: kn %g, kz %g, ka %g\n", (double)guide_params.kn, (double)guide_params.kz,
                        (double)guide_params.ka);
        if (rts_save_png(rgba.data(), width, height, output.c_str()) != 0)
            uncaught("java.lang.RuntimeException", "Failed to save texture as PNG");
        char abs_path[PATH_MAX];
        const char* shown = realpath(output.c_str(), abs_path) ? abs_path : output.c_str();
        std::printf("A PNG file has been saved to: %s\n", shown);
    }
    if (!raw_output.empty()) {
        std::vector<float> rgba((size_t)width * height * 4);
        chk(rt_read_image(ctx, rgba.data()), "rt_read_image");
        if (rts_save_png(rgba.data(), width, height, raw_output.c_str()) != 0)
            uncaught("java.lang.RuntimeException", "Failed to save texture as PNG");
        char abs_path[PATH_MAX];
        const char* shown = realpath(raw_output.c_str(), abs_path) ? abs_path : raw_output.c_str();
        std::printf("The unfiltered image has been saved to: %s\n", shown);
    }
    if (!features_output.empty()) {
        // normal: N * 0.5 + 0.5; depth: t over the largest hit t, a miss black (both as bytes, no tonemap);
        // albedo: through the image's tonemap
        const size_t n = (size_t)width * height;
        std::vector<float> nd(n * 4), ai(n * 4);
        chk(rt_read_features(ctx, nd.data(), ai.data()), "rt_read_features");
        float tmax = 0.0f;
        for (size_t i = 0; i < n; i++)
            if (nd[i * 4 + 3] > tmax && nd[i * 4 + 3] <= 3.0e38f) tmax = nd[i * 4 + 3];
        auto byte_of = [](float v) { return (uint8_t)(v <= 0.0f ? 0 : v >= 1.0f ? 255 : (int)(v * 255.0f + 0.5f)); };
        std::vector<uint8_t> nrm(n * 3), dep(n * 3);
        for (size_t i = 0; i < n; i++) {
            const float t = nd[i * 4 + 3];
            const uint8_t z = (t > 0.0f && tmax > 0.0f && t <= tmax) ? byte_of(t / tmax) : 0;
            for (int c = 0; c < 3; c++) {
                nrm[i * 3 + c] = byte_of(nd[i * 4 + c] * 0.5f + 0.5f);
                dep[i * 3 + c] = z;
            }
            ai[i * 4 + 3] = 1.0f;   // (the id's bits are not a colour)
        }
        const std::string names[3] = {features_output + "_normal.png", features_output + "_albedo.png",
                                      features_output + "_depth.png"};
        if (rts_save_png_rgb8(nrm.data(), width, height, names[0].c_str()) != 0 ||
            rts_save_png(ai.data(), width, height, names[1].c_str()) != 0 ||
            rts_save_png_rgb8(dep.data(), width, height, names[2].c_str()) != 0)
            uncaught("java.lang.RuntimeException", "Failed to save texture as PNG");
        for (const std::string& nm : names) {
            char abs_path[PATH_MAX];
            const char* shown = realpath(nm.c_str(), abs_path) ? abs_path : nm.c_str();
            std::printf("A first-hit feature image has been saved to: %s\n", shown);
        }
    }
    if (moving) {
        // the poses: rt_render_moved each, the presented frame out as 4 bytes per pixel
        const size_t n = (size_t)width * height;
        const size_t dot = output.rfind('.');
        const bool has_ext = dot != std::string::npos && output.find('/', dot) == std::string::npos && dot > 0;
        const std::string stem = has_ext ? output.substr(0, dot) : output;
        // the pose's own, then the refinement's (--move-noise: every round's, rendered or not)
        const int pose_frames = move_frames + (noise_moves ? move_noise_batch * move_noise_rounds : move_refine);
        std::vector<float> mrf((size_t)pose_frames);
        rt_refine_params refine;
        std::memset(&refine, 0, sizeof(refine));
        refine.min_count = move_refine_count;
        refine.extra_frames = move_refine;
        refine.max_tiles = move_refine_tiles;
        int n_tiles = 0;
        if (move_refine || noise_moves) chk(rt_read_tile_frames(ctx, nullptr, 0, &n_tiles), "rt_read_tile_frames");
        rt_noise_refine_params to_noise;
        std::memset(&to_noise, 0, sizeof(to_noise));
        to_noise.target_noise = move_noise;
        to_noise.min_count = move_noise_count;
        to_noise.batch_frames = move_noise_batch;
        to_noise.max_rounds = move_noise_rounds;
        std::vector<uint8_t> rgba8(n * 4), rgb8(n * 3);
        const float step = (float)((double)move_shift * width);
        for (int k = 1; k <= moves; k++) {
            for (int c = 0; c < 3; c++) {
                const float v = ubo[12 + c] * step;
                ubo[4 + c] += v;
                ubo[8 + c] += v;
            }
            for (int i = 0; i < pose_frames; i++)
                mrf[(size_t)i] = rt_frame_rand_factor((uint64_t)seed, (uint64_t)spp + (uint64_t)(k - 1) * pose_frames + i);
            int refined = 0, rounds = 0;
            int64_t spent = 0;
            rt_moved_noise_stats mstats;
            std::memset(&mstats, 0, sizeof(mstats));
            if (noise_moves)
                chk(rt_render_moved_to_noise(ctx, ubo, move_frames, mrf.data(), &to_noise, nullptr, nullptr, nullptr, nullptr, &rounds,
                                             &refined, &spent, &mstats),
                    "rt_render_moved_to_noise");
            else if (move_refine)
                chk(rt_render_moved_refined(ctx, ubo, move_frames, mrf.data(), &refine, nullptr, nullptr, nullptr, nullptr, &refined),
                    "rt_render_moved_refined");
            else
                chk(rt_render_moved(ctx, ubo, move_frames, mrf.data(), nullptr, nullptr, nullptr, nullptr), "rt_render_moved");
            chk(rt_read_presented(ctx, rgba8.data()), "rt_read_presented");
            for (size_t i = 0; i < n; i++)
                for (int c = 0; c < 3; c++) rgb8[i * 3 + c] = rgba8[i * 4 + c];
            char num[32];
            std::snprintf(num, sizeof(num), ".move%02d.png", k);
            const std::string name = stem + num;
            if (rts_save_png_rgb8(rgb8.data(), width, height, name.c_str()) != 0)
                uncaught("java.lang.RuntimeException", "Failed to save texture as PNG");
            char abs_path[PATH_MAX];
            const char* shown = realpath(name.c_str(), abs_path) ? abs_path : name.c_str();
            if (noise_moves)
                std::printf("Move %d/%d: %d frame(s), +%lld tile-frame(s) in %d round(s) on %d of %d tiles, noise %.6g (%s), saved to: %s\n",
                            k, moves, move_frames, (long long)spent, rounds, refined, n_tiles, mstats.noise,
                            mstats.converged ? "converged" : "round cap reached", shown);
            else if (move_refine)
                std::printf("Move %d/%d: %d frame(s), +%d on %d of %d tiles, saved to: %s\n", k, moves, move_frames, move_refine,
                            refined, n_tiles, shown);
            else
                std::printf("Move %d/%d: %d frame(s), saved to: %s\n", k, moves, move_frames, shown);
        }
    }
    rt_destroy(ctx);
    rts_free(scene);
    return 0;
}
