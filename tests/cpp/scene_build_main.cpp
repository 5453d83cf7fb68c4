// Stand-alone checker of what the scene upload decides before it touches the GPU
// (eray_amd/csrc/scene_build.hpp and texel_prog.hpp, the headers capi_scene.cpp's sync_scene and
// the kernels share): plain host code, no library to link, meant for the host sanitizers and a
// machine without a GPU:
//
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tests/cpp/scene_build_main.cpp -o /tmp/scene_build && /tmp/scene_build
//
// Every expectation is a plain restatement written here, never the headers' own function:
//   graphs       seeded random shader graphs (as tests/test_gpu_texel_graph.py random_graph makes
//                them) run as Graph::run does — every node's whole image by the node formulas, the
//                wave's with the host's cosf — against the compiled program evaluated by
//                texel_program, the function the kernels run, on f32 bit patterns; the trees' sizes
//                against a restated count (rgb's identical inputs share one child), which also says
//                which graphs are refused;
//   limit        flat + 4 / 5 mixes of (i, i): 31 instructions compile, 63 are refused;
//   validation   every rejecting branch of check_texel_graph with its status and exact message;
//   descriptors  build_scene_descs field by field, scene_reflective;
//   raw layout   raw_slices tiles the scene's array and packs / unpacks the objects' arrays.
// (f32 as the kernels compute it: no fused multiply-add — g++'s default for x86-64.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../eray_amd/csrc/scene_build.hpp"

using namespace eray::gpu;

namespace {
int g_failed = 0;
long g_checks = 0;
constexpr size_t kWhy = 256;  // (the messages' buffer, as the scene call's)
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++g_checks;                                       \
        if (!(cond)) {                                    \
            if (++g_failed <= 40) {                       \
                std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
    uint32_t range(uint32_t lo, uint32_t hi) { return lo + below(hi - lo + 1); }  // inclusive
    float uniform(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
};

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

eray_texel_node node(uint32_t kind, uint32_t w, uint32_t h, float p0 = 0, float p1 = 0, float p2 = 0, int32_t i0 = -1,
                     int32_t i1 = -1, int32_t i2 = -1) {
    eray_texel_node n{};
    n.kind = kind;
    n.width = w;
    n.height = h;
    n.param[0] = p0;
    n.param[1] = p1;
    n.param[2] = p2;
    n.input[0] = i0;
    n.input[1] = i1;
    n.input[2] = i2;
    return n;
}
bool is_wave(const eray_texel_node& n) { return n.kind == ERAY_TEXEL_WAVE; }

// ---- graphs against Graph::run
// tests/test_gpu_texel_graph.py random_graph: a wave, a flat colour, then any node whose inputs exist;
// rgb's inputs are waves of no fewer pixels (30 %: one wave three times), mix factors in [-0.2, 1.2].
std::vector<eray_texel_node> random_graph(Rng& rng, uint32_t n_nodes) {
    std::vector<eray_texel_node> g;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        std::vector<int32_t> waves, colors;
        for (uint32_t j = 0; j < i; ++j) (is_wave(g[j]) ? waves : colors).push_back((int32_t)j);
        std::vector<uint32_t> choices{ERAY_TEXEL_WAVE, ERAY_TEXEL_FLAT_COLOR};
        if (!waves.empty()) choices.push_back(ERAY_TEXEL_RGB);
        if (!colors.empty()) choices.push_back(ERAY_TEXEL_MIX_COLOR);
        const uint32_t kind = i == 0 ? ERAY_TEXEL_WAVE : i == 1 ? ERAY_TEXEL_FLAT_COLOR : choices[rng.below((uint32_t)choices.size())];
        uint32_t w = rng.range(3, 39), h = rng.range(3, 39);
        if (kind == ERAY_TEXEL_WAVE) {
            g.push_back(node(kind, w, h, rng.uniform(-3, 3), rng.uniform(-3, 3)));
        } else if (kind == ERAY_TEXEL_FLAT_COLOR) {
            g.push_back(node(kind, w, h, rng.uniform(0, 1.2f), rng.uniform(0, 1.2f), rng.uniform(0, 1.2f)));
        } else if (kind == ERAY_TEXEL_RGB) {
            int32_t in[3];
            for (int k = 0; k < 3; ++k) in[k] = waves[rng.below((uint32_t)waves.size())];
            if (rng.below(10) < 3) in[1] = in[2] = in[0];
            uint32_t min_w = ~0u, min_px = ~0u;
            for (int k = 0; k < 3; ++k) {
                min_w = std::min(min_w, g[in[k]].width);
                min_px = std::min(min_px, g[in[k]].width * g[in[k]].height);
            }
            w = std::min(w, min_w);
            h = std::max(std::min(h, min_px / w), 1u);
            g.push_back(node(kind, w, h, 0, 0, 0, in[0], in[1], in[2]));
        } else {
            const int32_t l = colors[rng.below((uint32_t)colors.size())], r = colors[rng.below((uint32_t)colors.size())];
            g.push_back(node(kind, w, h, rng.uniform(-0.2f, 1.2f), 0, 0, l, r));
        }
    }
    return g;
}

// A node's image as the reference's node makes it: w * h pixels of 1 (wave) or 3 floats.
struct Image {
    uint32_t w, h, comps;
    std::vector<float> px;
    const float* mod_get(uint32_t x, uint32_t y) const { return &px[comps * ((size_t)(y % h) * w + x % w)]; }  // image.rs:36-38
};
std::vector<Image> run_graph(const std::vector<eray_texel_node>& g) {
    std::vector<Image> img;
    for (const eray_texel_node& n : g) {
        Image im{n.width, n.height, is_wave(n) ? 1u : 3u, {}};
        im.px.resize((size_t)im.comps * n.width * n.height);
        for (uint32_t y = 0; y < n.height; ++y)
            for (uint32_t x = 0; x < n.width; ++x) {
                const size_t i = (size_t)y * n.width + x;
                if (n.kind == ERAY_TEXEL_WAVE) {  // wave.rs:127
                    const float arg = ((float)x * n.param[0] + (float)y * n.param[1]) / 10.0f;
                    im.px[i] = std::fabs(cosf(arg));
                } else if (n.kind == ERAY_TEXEL_RGB) {  // rgb.rs:89-95: the inputs' pixels at the node's index
                    for (int c = 0; c < 3; ++c) im.px[3 * i + c] = img[n.input[c]].px[i];
                } else if (n.kind == ERAY_TEXEL_FLAT_COLOR) {
                    for (int c = 0; c < 3; ++c) im.px[3 * i + c] = n.param[c];
                } else {  // mix_color.rs:85-91
                    const float *l = img[n.input[0]].mod_get(x, y), *r = img[n.input[1]].mod_get(x, y), f = n.param[0];
                    for (int c = 0; c < 3; ++c) im.px[3 * i + c] = l[c] * (1.0f - f) + r[c] * f;
                }
            }
        img.push_back(std::move(im));
    }
    return img;
}
// Rust's `x as u32`
uint32_t as_u32(float f) {
    if (std::isnan(f) || f <= 0.0f) return 0u;
    if (f >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)f;
}
// The instructions of node idx's tree: a mix has both children, an rgb one child per distinct input.
uint64_t tree_size(const std::vector<eray_texel_node>& g, int32_t idx) {
    const eray_texel_node& n = g[idx];
    uint64_t s = 1;
    if (n.kind == ERAY_TEXEL_MIX_COLOR) s += tree_size(g, n.input[0]) + tree_size(g, n.input[1]);
    if (n.kind == ERAY_TEXEL_RGB)
        for (int j = 0; j < 3; ++j) {
            bool seen = false;
            for (int q = 0; q < j; ++q) seen = seen || n.input[q] == n.input[j];
            if (!seen) s += tree_size(g, n.input[j]);
        }
    return s;
}

// Output `out` of the graph set to node `idx`: the compiled program against the node's image.
void check_output(const std::vector<eray_texel_node>& g, const std::vector<Image>& img, int out, int32_t idx, uint64_t seed) {
    int32_t tout[5] = {-1, -1, -1, -1, -1};
    tout[out] = idx;
    std::vector<uint32_t> words{0xabcdef01u, 7u};  // (the program is appended)
    const int refused = compile_texel_program(g, tout, words);
    const bool typed = !is_wave(g[idx]) == (out == 0);
    const uint64_t size = tree_size(g, idx);
    if (typed && size > kTexelMaxNodes) {
        CHECK(refused == out && words.size() == 2, "seed %llu output %d: a tree of %llu instructions, refused %d",
              (unsigned long long)seed, out, (unsigned long long)size, refused);
        return;
    }
    CHECK(refused == -1 && words.size() >= 2 + kTexelHeaderWords && words[0] == 0xabcdef01u && words[1] == 7u,
          "seed %llu output %d: refused %d", (unsigned long long)seed, out, refused);
    if (refused != -1) return;
    const uint32_t* prog = words.data() + 2;
    for (int o = 0; o < 5; ++o) {
        const uint32_t want = o == out && typed ? (uint32_t)size : 0u;
        CHECK(prog[5 + o] == want, "seed %llu output %d: count[%d] = %u, tree %u", (unsigned long long)seed, out, o, prog[5 + o], want);
    }
    CHECK(words.size() == 2 + kTexelHeaderWords + (typed ? size : 0) * 12, "seed %llu output %d: %zu words", (unsigned long long)seed,
          out, words.size());
    float val[3] = {-1.0f, -1.0f, -1.0f};
    if (!typed) {  // a wave as color, a colour node as a scalar: Material::get reads None
        CHECK(!texel_program(prog, (uint32_t)out, 0.5f, 0.5f, val), "seed %llu: mistyped output %d evaluates", (unsigned long long)seed, out);
        return;
    }
    const Image& im = img[idx];
    const auto at = [&](float u, float v) {
        const bool ok = texel_program(prog, (uint32_t)out, u, v, val);
        const float* want = im.mod_get(as_u32(u * (float)im.w), as_u32(v * (float)im.h));  // material.rs:56-94
        bool same = ok;
        for (uint32_t c = 0; c < im.comps; ++c) same = same && bits(val[c]) == bits(want[c]);
        CHECK(same, "seed %llu output %d node %d at uv (%g, %g): got %08x, image %08x", (unsigned long long)seed, out, idx, u, v,
              bits(val[0]), bits(want[0]));
        for (int o = 0; o < 5; ++o)
            if (o != out) CHECK(!texel_program(prog, (uint32_t)o, u, v, val), "output %d is no program output", o);
    };
    for (uint32_t y = 0; y < im.h; ++y)
        for (uint32_t x = 0; x < im.w; ++x) at(((float)x + 0.5f) / (float)im.w, ((float)y + 0.5f) / (float)im.h);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float odd[6] = {-0.25f, 1.0f, 7.3f, 1e10f, inf, nan};  // the saturating cast and the wrap
    for (float u : odd)
        for (float v : odd) at(u, v);
}

void random_graphs() {
    uint64_t compiled = 0, refused = 0;
    for (uint64_t seed = 1; seed <= 240; ++seed) {
        Rng rng{seed * 0x51ed27ull};
        const std::vector<eray_texel_node> g = random_graph(rng, 2 + (uint32_t)(seed % 7));
        eray_texel_graph tg{g.data(), (uint32_t)g.size(), -1, -1, -1, -1, -1};
        char why[kWhy];
        CHECK(check_texel_graph(&tg, why, sizeof why) == ERAY_OK, "seed %llu: a valid graph is refused: %s", (unsigned long long)seed, why);
        const std::vector<Image> img = run_graph(g);
        int32_t color = -1, wave = -1;  // the last colour node (the deepest tree) and some wave
        std::vector<int32_t> waves;
        for (size_t j = 0; j < g.size(); ++j) {
            if (is_wave(g[j])) waves.push_back((int32_t)j);
            else color = (int32_t)j;
        }
        wave = waves[rng.below((uint32_t)waves.size())];
        (tree_size(g, color) > kTexelMaxNodes ? refused : compiled) += 1;
        for (int out = 0; out < 5; ++out)
            for (int32_t idx : {color, wave}) check_output(g, img, out, idx, seed);
    }
    CHECK(compiled >= 200, "%llu random graphs compiled (%llu refused)", (unsigned long long)compiled, (unsigned long long)refused);
}

// rgb's inputs at the same node read the same pixel index: one child serves them.
void rgb_sharing() {
    const eray_texel_node w0 = node(ERAY_TEXEL_WAVE, 8, 8, 1, 2), w1 = node(ERAY_TEXEL_WAVE, 9, 8, 2, 1), w2 = node(ERAY_TEXEL_WAVE, 8, 9, 3, 1);
    struct Case { int32_t in[3]; uint32_t count; uint32_t child[3]; };
    for (const Case& c : {Case{{0, 0, 0}, 2, {1, 1, 1}}, Case{{0, 1, 0}, 3, {1, 2, 1}}, Case{{0, 0, 1}, 3, {1, 1, 2}},
                          Case{{1, 0, 0}, 3, {1, 2, 2}}, Case{{0, 1, 2}, 4, {1, 2, 3}}}) {
        const std::vector<eray_texel_node> g{w0, w1, w2, node(ERAY_TEXEL_RGB, 4, 4, 0, 0, 0, c.in[0], c.in[1], c.in[2])};
        const int32_t tout[5] = {3, -1, -1, -1, -1};
        std::vector<uint32_t> words;
        CHECK(compile_texel_program(g, tout, words) == -1, "rgb compiles");
        CHECK(words.size() == kTexelHeaderWords + 12u * c.count && words[0] == 0 && words[5] == c.count,
              "rgb (%d, %d, %d): %u instructions", c.in[0], c.in[1], c.in[2], words.size() > 5 ? words[5] : 0u);
        if (words.size() != kTexelHeaderWords + 12u * c.count) continue;
        const TexelInstr* ins = reinterpret_cast<const TexelInstr*>(words.data() + kTexelHeaderWords);
        CHECK(ins[0].kind == ERAY_TEXEL_RGB && ins[0].parent == 0 && ins[0].xform == kTexelMod, "the root");
        for (int j = 0; j < 3; ++j) {
            const TexelInstr& ch = ins[c.child[j]];
            CHECK(ins[0].c[j] == c.child[j] && ch.kind == ERAY_TEXEL_WAVE && ch.w == g[c.in[j]].width && ch.h == g[c.in[j]].height &&
                      ch.parent == 0 && ch.xform == kTexelIndex, "rgb (%d, %d, %d): child %d", c.in[0], c.in[1], c.in[2], j);
        }
    }
}

// ---- the expansion limit.  (sync_scene reports a refused output i of object o as
// "object %zu: output %d expands to more than %u texel nodes" with o, i and kTexelMaxNodes,
// status ERAY_E_UNSUPPORTED.)
void expansion_limit() {
    CHECK(kTexelMaxNodes == 32, "the node limit the message names");
    for (int mixes : {4, 5}) {
        std::vector<eray_texel_node> g{node(ERAY_TEXEL_WAVE, 4, 4, 1, 1), node(ERAY_TEXEL_FLAT_COLOR, 4, 4, 1, 0, 0)};
        for (int i = 0; i < mixes; ++i) g.push_back(node(ERAY_TEXEL_MIX_COLOR, 4, 4, 0.5f, 0, 0, 1 + i, 1 + i));
        const int32_t tout[5] = {(int32_t)g.size() - 1, 0, 0, -1, -1};
        std::vector<uint32_t> words{1u, 2u, 3u};
        const int refused = compile_texel_program(g, tout, words);
        if (mixes == 4) {
            CHECK(refused == -1 && words.size() == 3 + kTexelHeaderWords + 12u * 33u, "31 + 1 + 1 instructions: refused %d, %zu words", refused,
                  words.size());
            CHECK(words[3 + 5] == 31 && words[3 + 6] == 1 && words[3 + 7] == 1 && words[3 + 0] == 0 && words[3 + 1] == 31 && words[3 + 2] == 32,
                  "the outputs' counts and first instructions");
        } else {
            CHECK(refused == 0 && words.size() == 3, "63 instructions: refused %d, %zu words", refused, words.size());
        }
    }
    // the limit itself: trees of 32 and 33 instructions (rgb of one wave is 2; mixes add 1)
    std::vector<eray_texel_node> g{node(ERAY_TEXEL_WAVE, 4, 4, 1, 1), node(ERAY_TEXEL_FLAT_COLOR, 4, 4, 1, 0, 0)};
    const auto mix = [&](int32_t l, int32_t r) {
        g.push_back(node(ERAY_TEXEL_MIX_COLOR, 4, 4, 0.5f, 0, 0, l, r));
        return (int32_t)g.size() - 1;
    };
    g.push_back(node(ERAY_TEXEL_RGB, 4, 4, 0, 0, 0, 0, 0, 0));  // node 2: 2 instructions
    const int32_t m1 = mix(1, 1), m2 = mix(m1, m1), m3 = mix(m2, m2);  // 3, 7, 15
    const int32_t a = mix(1, 2), b = mix(m1, a), c = mix(m2, b);      // 4, 8, 16
    const int32_t d32 = mix(m3, c), d33 = mix(c, c);
    CHECK(tree_size(g, d32) == 32 && tree_size(g, d33) == 33, "the trees' sizes");
    for (int32_t root : {d32, d33}) {
        const int32_t tout[5] = {root, -1, -1, -1, -1};
        std::vector<uint32_t> words;
        const int refused = compile_texel_program(g, tout, words);
        if (root == d32)
            CHECK(refused == -1 && words.size() == kTexelHeaderWords + 12u * 32u && words[5] == 32, "32 instructions compile: refused %d", refused);
        else
            CHECK(refused == 0 && words.empty(), "33 instructions are refused: %d", refused);
    }
}

// ---- validation
constexpr int kOutNames = 5;
void expect(const std::vector<eray_texel_node>& nodes, std::initializer_list<int32_t> outs, int status, const char* message) {
    eray_texel_graph g{nodes.data(), (uint32_t)nodes.size(), -1, -1, -1, -1, -1};
    int32_t* slot[kOutNames] = {&g.color, &g.diffuse, &g.specular, &g.specular_power, &g.reflection};
    int k = 0;
    for (int32_t o : outs) *slot[k++] = o;
    char why[kWhy];
    std::memset(why, '#', sizeof why);
    const int st = check_texel_graph(&g, why, sizeof why);
    CHECK(std::memchr(why, 0, sizeof why) != nullptr, "the message is terminated");
    CHECK(st == status && std::strcmp(why, message) == 0, "status %d (want %d), message '%.100s' (want '%s')", st, status, why, message);
    // and the scene call's host half: a refused graph leaves the object's as it was
    HostObject o;
    o.tnodes.assign(3, node(ERAY_TEXEL_WAVE, 2, 2));
    o.tout[2] = 1;
    char why2[kWhy];
    CHECK(set_texel_graph(o, &g, why2, sizeof why2) == status && std::strcmp(why2, message) == 0, "set_texel_graph: '%s'", why2);
    if (status != ERAY_OK) {
        CHECK(o.tnodes.size() == 3 && o.tout[2] == 1 && o.tout[0] == -1, "a refused graph changes the object");
    } else {
        bool same = o.tnodes.size() == nodes.size() && (nodes.empty() || !std::memcmp(o.tnodes.data(), nodes.data(), sizeof(eray_texel_node) * nodes.size()));
        k = 0;
        for (int32_t* s : slot) same = same && o.tout[k++] == *s;
        CHECK(same, "an accepted graph is kept");
    }
}
void validation() {
    const eray_texel_node wave = node(ERAY_TEXEL_WAVE, 4, 4, 1, 1), flat = node(ERAY_TEXEL_FLAT_COLOR, 4, 4, 1, 0, 0);
    {  // null nodes with a count
        eray_texel_graph g{nullptr, 2, -1, -1, -1, -1, -1};
        char why[kWhy];
        CHECK(check_texel_graph(&g, why, sizeof why) == ERAY_E_INVALID_ARGUMENT && !std::strcmp(why, "nodes is null"), "'%s'", why);
    }
    expect({}, {}, ERAY_OK, "");
    expect({wave, flat}, {1, 0, 0, 0, 0}, ERAY_OK, "");
    expect({wave, node(4, 4, 4)}, {}, ERAY_E_INVALID_ARGUMENT, "node 1: kind 4");
    expect({node(ERAY_TEXEL_WAVE, 0, 4)}, {}, ERAY_E_OUT_OF_BOUNDS, "node 0: zero width or height");
    expect({wave, flat, node(ERAY_TEXEL_FLAT_COLOR, 4, 0)}, {}, ERAY_E_OUT_OF_BOUNDS, "node 2: zero width or height");
    expect({wave, node(ERAY_TEXEL_RGB, 4, 4, 0, 0, 0, 0, -1, 0)}, {}, ERAY_E_MISSING_MANY, "node 1: input 1 is not an earlier node");
    expect({wave, node(ERAY_TEXEL_RGB, 4, 4, 0, 0, 0, 0, 0, 1)}, {}, ERAY_E_MISSING_MANY, "node 1: input 2 is not an earlier node");
    expect({wave, flat, node(ERAY_TEXEL_MIX_COLOR, 4, 4, 0.5f, 0, 0, 3, 1), flat}, {}, ERAY_E_MISSING_MANY,
           "node 2: input 0 is not an earlier node");
    expect({flat, node(ERAY_TEXEL_RGB, 4, 4, 0, 0, 0, 0, 0, 0)}, {}, ERAY_E_INVALID_TYPE, "node 1: input 0 has the wrong image type");
    expect({flat, wave, node(ERAY_TEXEL_MIX_COLOR, 4, 4, 0.5f, 0, 0, 0, 1)}, {}, ERAY_E_INVALID_TYPE,
           "node 2: input 1 has the wrong image type");
    expect({node(ERAY_TEXEL_WAVE, 5, 3), node(ERAY_TEXEL_RGB, 4, 4, 0, 0, 0, 0, 0, 0)}, {}, ERAY_E_OUT_OF_BOUNDS,
           "node 1: input 0 has fewer pixels than the node");  // 15 pixels for 16
    expect({node(ERAY_TEXEL_WAVE, 8, 2), node(ERAY_TEXEL_RGB, 4, 4, 0, 0, 0, 0, 0, 0)}, {}, ERAY_OK, "");  // 16 for 16
    for (int k = 0; k < 5; ++k)
        for (int32_t bad : {-2, 2}) {
            char msg[64];
            std::snprintf(msg, sizeof msg, "output %d: node %d out of range", k, bad);
            int32_t outs[5] = {-1, -1, -1, -1, -1};
            outs[k] = bad;
            expect({wave, flat}, {outs[0], outs[1], outs[2], outs[3], outs[4]}, ERAY_E_INVALID_ARGUMENT, msg);
        }
    // the first rejecting branch decides (node order, then the outputs)
    expect({wave, node(9, 0, 0)}, {7}, ERAY_E_INVALID_ARGUMENT, "node 1: kind 9");
    // a null graph removes the object's
    HostObject o;
    o.tnodes.assign(2, wave);
    o.tout[0] = 1;
    o.tout[4] = 0;
    char why[kWhy] = "#";
    CHECK(set_texel_graph(o, nullptr, why, sizeof why) == ERAY_OK && !why[0], "a null graph");
    bool cleared = o.tnodes.empty();
    for (int32_t t : o.tout) cleared = cleared && t == -1;
    CHECK(cleared, "a null graph clears the object's graph");
}

// ---- descriptors
bool same_tex(const TexView& a, const float* data, uint32_t w, uint32_t h) { return a.data == data && a.w == w && a.h == h; }
void descriptors() {
    static float texels[16];
    std::vector<uint32_t> progs(4096);
    const uint32_t face_counts[5] = {0, 1, 256, 257, 1000};
    Rng rng{2024};
    for (uint32_t nobj : {0u, 1u, 3u, 17u, 17u, 17u})
        for (uint32_t nlights = 0; nlights <= 3; ++nlights) {
            std::vector<HostObject> objs(nobj);
            std::vector<size_t> prog_at(nobj, SIZE_MAX);
            for (uint32_t i = 0; i < nobj; ++i) {
                HostObject& o = objs[i];
                o.T = face_counts[nobj == 1 ? nlights + 1 : rng.below(5)];
                for (int k = 0; k < 3; ++k) {
                    o.lo[k] = rng.uniform(-5, 0);
                    o.hi[k] = rng.uniform(0, 5);
                }
                eray_image* im[5] = {&o.mat.color, &o.mat.diffuse, &o.mat.specular, &o.mat.specular_power, &o.mat.reflection};
                for (int k = 0; k < 5; ++k)
                    if (rng.below(2)) *im[k] = eray_image{texels + k, 10u + (uint32_t)k + i, 20u + (uint32_t)k};
                if (rng.below(3) == 0) {
                    o.example = true;
                    o.ex = eray_material_example_params{64u + i, 32u + i, 1.5f, 2.5f, 0.1f, 0.2f, 0.3f, 0.4f + (float)i};
                }
                if (rng.below(3) == 0) {  // a graph: wave, flat, wave; outputs kept, typed or mistyped
                    o.tnodes = {node(ERAY_TEXEL_WAVE, 4, 4, 1, 1), node(ERAY_TEXEL_FLAT_COLOR, 4, 4, 1, 0, 0), node(ERAY_TEXEL_WAVE, 2, 2, 1, 1)};
                    for (int k = 0; k < 5; ++k) o.tout[k] = (int32_t)rng.below(4) - 1;
                    prog_at[i] = 100 * (size_t)i + 12;
                }
            }
            std::vector<eray_light> lights(nlights);
            for (uint32_t l = 0; l < nlights; ++l)
                lights[l] = eray_light{{1.0f + l, 2.0f, 3.0f}, (int32_t)((l + nobj) % 2), {0.25f, 0.5f + l, 0.75f}, 10.0f + l};
            SceneDescs d;
            d.objs.resize(3);  // (what an earlier upload left)
            d.lights.resize(5);
            d.binned = 9;
            d.spec_pow = d.example_mat = true;
            build_scene_descs(objs, lights, progs.data(), prog_at, d);

            CHECK(d.objs.size() == nobj && d.lights.size() == nlights && d.begin.size() == 2 * (size_t)nobj + 1, "%u objects, %u lights", nobj,
                  nlights);
            if (d.objs.size() != nobj || d.lights.size() != nlights || d.begin.size() != 2 * (size_t)nobj + 1) continue;
            uint32_t begin = 0, binned = 0;
            bool spec_pow = false, example_mat = false;
            for (uint32_t i = 0; i < nobj; ++i) {
                const HostObject& o = objs[i];
                const ObjectDesc& e = d.objs[i];
                const bool graph = prog_at[i] != SIZE_MAX;
                CHECK(e.g.tri_begin == begin && e.g.tri_count == o.T && d.begin[i] == begin, "object %u: faces [%u, +%u)", i, e.g.tri_begin,
                      e.g.tri_count);
                CHECK(e.g.rect[0] == 0 && e.g.rect[1] == INT32_MAX && e.g.rect[2] == 0 && e.g.rect[3] == INT32_MAX, "object %u: every pixel", i);
                for (int k = 0; k < 3; ++k) CHECK(bits(e.g.bb_lo[k]) == bits(o.lo[k]) && bits(e.g.bb_hi[k]) == bits(o.hi[k]), "object %u: box", i);
                CHECK(e.g.bin_start == nullptr && e.g.bin_ent == nullptr, "object %u: no bins yet", i);
                const eray_image* im[5] = {&o.mat.color, &o.mat.diffuse, &o.mat.specular, &o.mat.specular_power, &o.mat.reflection};
                const TexView* tv[5] = {&e.mat.color, &e.mat.diffuse, &e.mat.specular, &e.mat.specular_power, &e.mat.reflection};
                for (int k = 0; k < 5; ++k) {
                    // the example material is color and diffuse; a graph's outputs replace the textures
                    const bool none = (o.example && k < 2) || (graph && o.tout[k] >= 0);
                    CHECK(none ? same_tex(*tv[k], nullptr, 0, 0) : same_tex(*tv[k], im[k]->data, im[k]->width, im[k]->height),
                          "object %u: texture %d (example %d, graph output %d)", i, k, (int)o.example, o.tout[k]);
                }
                if (o.example)
                    CHECK(e.mat.example == 1 && e.mat.ex_w == o.ex.width && e.mat.ex_h == o.ex.height && e.mat.ex_xf == o.ex.x_fac &&
                              e.mat.ex_yf == o.ex.y_fac && e.mat.ex_r == o.ex.r && e.mat.ex_g == o.ex.g && e.mat.ex_b == o.ex.b &&
                              e.mat.ex_factor == o.ex.factor, "object %u: the example material's parameters", i);
                else
                    CHECK(e.mat.example == 0 && e.mat.ex_w == 0 && e.mat.ex_h == 0 && e.mat.ex_xf == 0 && e.mat.ex_yf == 0 && e.mat.ex_r == 0 &&
                              e.mat.ex_g == 0 && e.mat.ex_b == 0 && e.mat.ex_factor == 0, "object %u: no example material", i);
                CHECK(e.mat.prog == (graph ? progs.data() + prog_at[i] : nullptr), "object %u: its program", i);
                CHECK(d.begin[nobj + 1 + i] == (o.T > 256 ? binned : ~0u), "object %u of %u faces: key %u", i, o.T, d.begin[nobj + 1 + i]);
                binned += o.T > 256;
                spec_pow = spec_pow || (graph && o.tout[3] >= 0 ? is_wave(o.tnodes[o.tout[3]]) : o.mat.specular_power.data != nullptr);
                example_mat = example_mat || o.example || graph;
                begin += o.T;
            }
            CHECK(d.begin[nobj] == begin, "all faces: %u", d.begin[nobj]);
            CHECK(d.binned == binned && d.spec_pow == spec_pow && d.example_mat == example_mat, "binned %u (%u), spec_pow %d (%d), example_mat %d (%d)",
                  d.binned, binned, (int)d.spec_pow, (int)spec_pow, (int)d.example_mat, (int)example_mat);
            for (uint32_t l = 0; l < nlights; ++l) {
                const LightDesc& e = d.lights[l];
                const eray_light& s = lights[l];
                CHECK(e.pos[0] == s.position[0] && e.pos[1] == s.position[1] && e.pos[2] == s.position[2] && e.variant == s.variant &&
                          e.color[0] == s.color[0] && e.color[1] == s.color[1] && e.color[2] == s.color[2] && e.brightness == s.brightness,
                      "light %u", l);
            }
        }
    // the kDirectMax boundary, whatever the draws above held
    std::vector<HostObject> objs(4);
    const uint32_t T[4] = {257, 256, 1000, 0};
    for (int i = 0; i < 4; ++i) objs[i].T = T[i];
    SceneDescs d;
    build_scene_descs(objs, {}, nullptr, std::vector<size_t>(4, SIZE_MAX), d);
    const uint32_t want[9] = {0, 257, 513, 1513, 1513, 0, ~0u, 1, ~0u};
    CHECK(d.begin.size() == 9 && !std::memcmp(d.begin.data(), want, sizeof want) && d.binned == 2, "obj_begin | objkey at 256 / 257 faces");
    // an example material over textures: color and diffuse go, the others stay
    objs.assign(1, HostObject{});
    objs[0].mat = eray_material{{texels, 2, 2}, {texels, 3, 3}, {texels, 4, 4}, {nullptr, 0, 0}, {texels, 6, 6}};
    objs[0].example = true;
    objs[0].ex = eray_material_example_params{8, 8, 1, 1, 1, 0, 0, 0.5f};
    build_scene_descs(objs, {}, nullptr, {SIZE_MAX}, d);
    CHECK(same_tex(d.objs[0].mat.color, nullptr, 0, 0) && same_tex(d.objs[0].mat.diffuse, nullptr, 0, 0) &&
              same_tex(d.objs[0].mat.specular, texels, 4, 4) && same_tex(d.objs[0].mat.reflection, texels, 6, 6) && d.example_mat && !d.spec_pow,
          "the example material clears color and diffuse");
    // specular power: a texture, a wave as graph output 3 (a colour node there reads None)
    for (int variant = 0; variant < 4; ++variant) {
        objs.assign(1, HostObject{});
        if (variant == 1) objs[0].mat.specular_power = eray_image{texels, 2, 2};
        if (variant >= 2) {
            objs[0].tnodes = {node(ERAY_TEXEL_WAVE, 4, 4, 1, 1), node(ERAY_TEXEL_FLAT_COLOR, 4, 4, 1, 0, 0)};
            objs[0].tout[3] = variant == 2 ? 0 : 1;
            objs[0].mat.specular_power = eray_image{texels, 2, 2};  // (replaced by the output)
        }
        build_scene_descs(objs, {}, progs.data(), {variant >= 2 ? (size_t)0 : SIZE_MAX}, d);
        CHECK(d.spec_pow == (variant == 1 || variant == 2) && d.example_mat == (variant >= 2), "specular power, variant %d", variant);
    }
    // scene_reflective: a reflection texture; graph output 4 a wave; a colour node there (None)
    objs.assign(2, HostObject{});
    CHECK(!scene_reflective(objs) && !scene_reflective({}), "nothing reflects");
    objs[1].mat.reflection = eray_image{texels, 2, 2};
    CHECK(scene_reflective(objs), "a reflection texture");
    objs[1].tnodes = {node(ERAY_TEXEL_WAVE, 4, 4, 1, 1), node(ERAY_TEXEL_FLAT_COLOR, 4, 4, 1, 0, 0)};
    objs[1].tout[4] = 1;
    CHECK(!scene_reflective(objs), "a colour node as the reflection output replaces the texture with None");
    objs[1].tout[4] = 0;
    objs[1].mat.reflection = eray_image{nullptr, 0, 0};
    CHECK(scene_reflective(objs), "a wave as the reflection output");
    objs[1].tout[4] = -1;
    CHECK(!scene_reflective(objs), "the output kept, no texture");
}

// ---- the raw arrays' layout
void raw_layout() {
    Rng rng{77};
    for (uint32_t total : {0u, 1u, 5u, 300u})
        for (uint32_t nobj = 1; nobj <= 4; ++nobj)
            for (int draw = 0; draw < 4; ++draw) {
                std::vector<uint32_t> T(nobj, 0);  // a split of the faces over the objects (empty ones too)
                for (uint32_t f = 0; f < total; ++f) ++T[draw == 0 ? f % nobj : rng.below(nobj)];
                std::vector<int> cover(24 * (size_t)total, 0);
                std::vector<float> scene(24 * (size_t)total, -1.0f);
                std::vector<std::vector<float>> own(nobj), back(nobj);
                uint32_t begin = 0;
                bool inside = true;
                for (uint32_t i = 0; i < nobj; ++i) {
                    own[i].resize(24 * (size_t)T[i]);
                    for (size_t k = 0; k < own[i].size(); ++k) own[i][k] = (float)(i * 100000 + k);
                    std::vector<int> cover_own(own[i].size(), 0);
                    const auto sl = raw_slices(total, begin, T[i]);
                    CHECK(sl[0].count == 9u * T[i] && sl[1].count == 9u * T[i] && sl[2].count == 6u * T[i], "slice lengths of %u faces", T[i]);
                    for (const RawSlice& s : sl) {
                        inside = inside && s.in_scene + s.count <= scene.size() && s.in_object + s.count <= own[i].size();
                        if (!inside) break;
                        for (size_t k = 0; k < s.count; ++k) {
                            ++cover[s.in_scene + k];
                            ++cover_own[s.in_object + k];
                            scene[s.in_scene + k] = own[i][s.in_object + k];  // pack
                        }
                    }
                    bool once = true;
                    for (int c : cover_own) once = once && c == 1;
                    CHECK(once, "an object's slices tile its own array (%u faces)", T[i]);
                    // the arrays' order, stated: all positions, then all normals, then all uvs, by face
                    for (uint32_t f = 0; f < T[i] && inside; ++f)
                        CHECK(scene[9 * (size_t)(begin + f)] == own[i][9 * (size_t)f] &&
                                  scene[9 * (size_t)total + 9 * (size_t)(begin + f) + 8] == own[i][9 * (size_t)T[i] + 9 * (size_t)f + 8] &&
                                  scene[18 * (size_t)total + 6 * (size_t)(begin + f) + 5] == own[i][18 * (size_t)T[i] + 6 * (size_t)f + 5],
                              "face %u of object %u in the scene's array", f, i);
                    begin += T[i];
                }
                CHECK(inside, "total %u over %u objects: a slice leaves its array", total, nobj);
                if (!inside) continue;
                bool once = true;
                for (int c : cover) once = once && c == 1;
                CHECK(once, "total %u over %u objects: the slices tile [0, 24 * total) once", total, nobj);
                begin = 0;
                for (uint32_t i = 0; i < nobj; ++i) {  // unpack
                    back[i].assign(own[i].size(), -2.0f);
                    for (const RawSlice& s : raw_slices(total, begin, T[i]))
                        for (size_t k = 0; k < s.count; ++k) back[i][s.in_object + k] = scene[s.in_scene + k];
                    CHECK(back[i] == own[i], "object %u's arrays return through the scene's", i);
                    begin += T[i];
                }
                // the whole scene as one object: the three arrays the record kernel reads
                const auto all = raw_slices(total, 0, total);
                CHECK(all[0].in_scene == 0 && all[1].in_scene == 9 * (size_t)total && all[2].in_scene == 18 * (size_t)total, "the scene's arrays");
            }
    CHECK(kRawFloatsPerFace == 24, "24 floats per face");
}

}  // namespace

int main() {
    random_graphs();
    rgb_sharing();
    expansion_limit();
    validation();
    descriptors();
    raw_layout();
    std::printf("scene_build: %ld checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
