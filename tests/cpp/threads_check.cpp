// threads_check -- the C ABI (include/volrend_hip.h) from concurrent host threads, on a real GPU.  Driven by
// tests/test_gpu_threads.py (and, for `errors`, tests/test_abi.py), which write the inputs and compare
// the outputs with the CPU yardsticks.
//
//   threads_check <mode> <dir>        mode: cold | mixed | uploads | devices | errors
// <dir> holds the inputs -- params.txt (`key value` lines), <tree>.meta / .child / .data (a tree in the file's
// layout; the meta line is N capacity data_dim format basis_dim offset[3] scale[3] n_quant n_retained, floats as
// their 32-bit patterns) and raw float32 arrays -- and receives the outputs: <dir>/<prefix><i>_<name>.raw is
// output <name> of thread i.
//
// Every thread owns its stream (non-blocking), its inputs and its output buffers, and synchronises only its own
// stream.  The threads start together behind a barrier.  Before EVERY library or HIP call a thread looks at one
// shared stop flag; the first call that returns non-zero sets it and prints the thread, the call and the text of
// vr_last_error(), so after an error nothing more is enqueued and the program exits with 1.  All round counts are
// fixed: nothing here loops until something happens.
//
// Built without HIP (tests/build_util.cpp_program(..., gpu=False)) only `errors` exists: it opens no device.
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "volrend_hip.h"

namespace {

std::atomic<bool> g_stop{false};
std::mutex g_print;

bool report(int thread, const char* call, int rc, const char* text) {
    g_stop.store(true);
    std::lock_guard<std::mutex> lock(g_print);
    printf("ERROR thread %d call %s returned %d: %s\n", thread, call, rc, text ? text : "");
    fflush(stdout);
    return false;
}

// `id` is the calling thread's number.  Both leave the enclosing function (which returns bool) on a set stop
// flag or a failed call.
#define VR(call)                                                              \
    do {                                                                      \
        if (g_stop.load()) return false;                                      \
        const int rc_ = (call);                                               \
        if (rc_ != 0) return report(id, #call, rc_, vr_last_error());         \
    } while (0)

class Barrier {
    std::mutex m_;
    std::condition_variable cv_;
    int waiting_ = 0, n_;
public:
    explicit Barrier(int n) : n_(n) {}
    void wait() {
        std::unique_lock<std::mutex> lock(m_);
        if (++waiting_ == n_) cv_.notify_all();
        else cv_.wait(lock, [this] { return waiting_ == n_; });
    }
};

// ---- errors: refusals and the thread-local vr_last_error, no device ------------------------------------------
// Thread i makes refusal kind i % 4 with a parameter of its own where the message has one, so that the texts of
// threads that run beside each other differ; each is refused before any tree is followed or any device call.
int refuse(int i) {
    static const int32_t child[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    static const uint16_t data[32] = {0};
    VrTreeDesc d;
    vr_default_tree_desc(&d);
    d.child = child;
    d.data = data;
    d.capacity = 1;
    d.data_dim = 4;
    vr_tree_t out = nullptr;
    switch (i % 4) {
        case 0: d.N = 1 - i / 4; return vr_tree_upload(&d, &out);        // "N=%d out of range"
        case 1: d.capacity = 0; return vr_tree_upload(&d, &out);         // "capacity must be positive"
        case 2: d.format = 7 + i; return vr_tree_upload(&d, &out);       // "unknown data format %d"
        default: return vr_reserve_rays(nullptr, 1000 + i, 1);           // "vr_reserve_rays: tree is NULL"
    }
}

int run_errors() {
    constexpr int kThreads = 8, kCalls = 2000;
    std::string expect[kThreads];
    int code[kThreads];
    for (int i = 0; i < kThreads; ++i) {   // each refusal alone, at start-up
        code[i] = refuse(i);
        expect[i] = vr_last_error();
        if (code[i] != VR_ERR_INVALID_ARGUMENT || expect[i].empty()) {
            printf("ERROR refusal %d alone returned %d: %s\n", i, code[i], expect[i].c_str());
            return 1;
        }
    }
    if (expect[0] == expect[4] || expect[2] == expect[6] || expect[0] == expect[1]) {
        printf("ERROR the refusals' texts do not differ\n");
        return 1;
    }
    Barrier barrier(kThreads);
    std::vector<std::thread> threads;
    for (int id = 0; id < kThreads; ++id)
        threads.emplace_back([&, id] {
            barrier.wait();
            for (int c = 0; c < kCalls; ++c) {
                if (g_stop.load()) return;
                const int rc = refuse(id);
                const char* text = vr_last_error();
                if (rc != code[id] || expect[id] != text) {
                    report(id, "refusal", rc, text);
                    return;
                }
            }
        });
    for (auto& t : threads) t.join();
    if (g_stop.load()) return 1;
    printf("calls %d\n", kThreads * kCalls);
    return 0;
}

}  // namespace

#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime.h>

namespace {

#define HIP(call)                                                                        \
    do {                                                                                 \
        if (g_stop.load()) return false;                                                 \
        const hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) return report(id, #call, (int)e_, hipGetErrorString(e_));  \
    } while (0)

std::string g_dir;
std::map<std::string, double> g_params;

double P(const std::string& key) {
    auto it = g_params.find(key);
    if (it == g_params.end()) {
        fprintf(stderr, "params.txt has no %s\n", key.c_str());
        exit(5);
    }
    return it->second;
}

template <typename T>
std::vector<T> read_file(const std::string& name, size_t count = 0) {
    std::ifstream f(g_dir + "/" + name, std::ios::binary | std::ios::ate);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", name.c_str());
        exit(5);
    }
    const size_t bytes = (size_t)f.tellg();
    if (bytes % sizeof(T) || (count && bytes != count * sizeof(T))) {
        fprintf(stderr, "%s: %zu bytes, expected %zu elements of %zu\n", name.c_str(), bytes, count, sizeof(T));
        exit(5);
    }
    std::vector<T> v(bytes / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
    return v;
}

struct HostTree {
    VrTreeDesc d;
    VrQuantDesc q;
    std::vector<int32_t> child;
    std::vector<uint16_t> data, qc, qm, sigma, ret;
    size_t slots() const { return (size_t)d.capacity * d.N * d.N * d.N; }
    size_t elems() const { return slots() * (size_t)d.data_dim; }
};

// <name>.meta / .child / .data (or, quantised, .qc / .qm / .sigma / .ret) -> the descriptors, pointing into `t`.
void load_tree(const std::string& name, HostTree& t) {
    std::ifstream m(g_dir + "/" + name + ".meta");
    long long v[13] = {};
    for (auto& x : v)
        if (!(m >> x)) {
            fprintf(stderr, "bad %s.meta\n", name.c_str());
            exit(5);
        }
    vr_default_tree_desc(&t.d);
    memset(&t.q, 0, sizeof(t.q));
    t.d.N = (int32_t)v[0];
    t.d.capacity = v[1];
    t.d.data_dim = (int32_t)v[2];
    t.d.format = (int32_t)v[3];
    t.d.basis_dim = (int32_t)v[4];
    for (int i = 0; i < 3; ++i) {
        const uint32_t o = (uint32_t)v[5 + i], s = (uint32_t)v[8 + i];
        memcpy(&t.d.offset[i], &o, 4);
        memcpy(&t.d.scale[i], &s, 4);
    }
    t.q.n_quant = (int32_t)v[11];
    t.q.n_retained = (int32_t)v[12];
    t.child = read_file<int32_t>(name + ".child", t.slots());
    t.d.child = t.child.data();
    if (t.q.n_quant + t.q.n_retained == 0) {
        t.data = read_file<uint16_t>(name + ".data", t.elems());
        t.d.data = t.data.data();
        return;
    }
    t.qc = read_file<uint16_t>(name + ".qc", (size_t)t.q.n_quant * 65536 * 3);
    t.qm = read_file<uint16_t>(name + ".qm", (size_t)t.q.n_quant * t.slots());
    t.sigma = read_file<uint16_t>(name + ".sigma", t.slots());
    t.q.quant_colors = t.qc.data();
    t.q.quant_map = t.qm.data();
    t.q.sigma = t.sigma.data();
    if (t.q.n_retained) {
        t.ret = read_file<uint16_t>(name + ".ret", (size_t)t.q.n_retained * t.slots() * 3);
        t.q.data_retained = t.ret.data();
    }
}

// The scenes' main tree goes up under top_levels = 2, brick_levels = 1 (top-grid, brick and child-word leaves in
// one tree); the process defaults are put back right after.
bool upload_main(const HostTree& h, vr_tree_t* out) {
    const int id = -1;
    VR(vr_set_tuning("top_levels", 2));
    VR(vr_set_tuning("brick_levels", 1));
    VR(vr_tree_upload(&h.d, out));
    VR(vr_set_tuning("top_levels", 0));
    VR(vr_set_tuning("brick_levels", 3));
    VrTreeInfo info;
    VR(vr_tree_info(*out, &info));
    printf("main_top_levels %d\nmain_brick_levels %d\n", info.top_levels, info.brick_levels);
    return true;
}

VrCamera camera(const float* pose, int w, int h, float f) {
    VrCamera c;
    memcpy(c.transform, pose, sizeof(c.transform));
    c.width = w;
    c.height = h;
    c.fx = c.fy = f;
    return c;
}

// One thread's script: its stream, its buffers, `rounds` calls, and its outputs as raw files.
struct Worker {
    int id = 0;
    int rounds = 4;
    bool finish_in_main = false;   // (devices: the thread's current device is not its stream's)
    hipStream_t stream = nullptr;
    std::vector<void*> owned;
    struct Out { std::string name; void* dev; size_t bytes; bool poison; };
    std::vector<Out> outs;

    virtual ~Worker() {   // in the main thread, after every thread has been joined
        for (void* p : owned) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
    virtual bool prepare() = 0;
    virtual bool call(int round) = 0;
    virtual bool after() { return true; }

    template <typename T>
    bool alloc(T** p, size_t count) {
        HIP(hipMalloc((void**)p, count * sizeof(T)));
        owned.push_back(*p);
        return true;
    }
    template <typename T>
    bool input(T** p, const std::vector<T>& host) {
        if (!alloc(p, host.size())) return false;
        HIP(hipMemcpy(*p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
        return true;
    }
    // An output of `count` elements.  poison: filled with 0xFF on the stream before every round (a call that
    // overwrites it); else zeroed once on the stream (a call that accumulates, or one slice per round).
    template <typename T>
    bool output(T** p, const std::string& name, size_t count, bool poison) {
        if (!alloc(p, count)) return false;
        HIP(hipMemsetAsync(*p, 0, count * sizeof(T), stream));
        outs.push_back({name, *p, count * sizeof(T), poison});
        return true;
    }
    bool setup() {
        HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return prepare();
    }
    bool run() {
        for (int r = 0; r < rounds; ++r) {
            for (const Out& o : outs)
                if (o.poison) HIP(hipMemsetAsync(o.dev, 0xFF, o.bytes, stream));
            if (!call(r)) return false;
        }
        return after();
    }
    bool finish(const std::string& prefix) {
        HIP(hipStreamSynchronize(stream));
        for (const Out& o : outs) {
            std::vector<char> host(o.bytes);
            HIP(hipMemcpyAsync(host.data(), o.dev, o.bytes, hipMemcpyDeviceToHost, stream));
            HIP(hipStreamSynchronize(stream));
            std::ofstream f(g_dir + "/" + prefix + std::to_string(id) + "_" + o.name + ".raw", std::ios::binary);
            f.write(host.data(), (std::streamsize)host.size());
            if (!f) return report(id, "write", 1, o.name.c_str());
        }
        return true;
    }
};

using Workers = std::vector<std::unique_ptr<Worker>>;

// Threaded: every worker in a thread of its own, all released together.  Serial: one after the other, here.
bool run_workers(Workers& ws, const std::string& prefix, bool threaded) {
    for (size_t i = 0; i < ws.size(); ++i) ws[i]->id = (int)i;
    if (!threaded) {
        for (auto& w : ws)
            if (!(w->setup() && w->run() && w->finish(prefix))) return false;
        return !g_stop.load();
    }
    Barrier barrier((int)ws.size());
    std::vector<std::thread> threads;
    for (auto& w : ws)
        threads.emplace_back([&barrier, &prefix, p = w.get()] {
            (void)p->setup();   // (a failure sets the stop flag; the thread still arrives at the barrier)
            barrier.wait();
            if (p->run() && !p->finish_in_main) (void)p->finish(prefix);
        });
    for (auto& t : threads) t.join();
    for (auto& w : ws)
        if (w->finish_in_main && !g_stop.load()) (void)w->finish(prefix);
    return !g_stop.load();
}

// ---- frames: vr_render_batch of n_frames poses into slices of one rgba and one accum buffer --------------------
struct FrameBuffers {
    uint8_t* rgba = nullptr;
    float* accum = nullptr;
    int w = 0, h = 0;
    size_t px() const { return (size_t)w * h; }
    VrFrame frame(int slice) const {
        VrFrame f;
        vr_default_frame(&f);
        f.rgba = rgba + (size_t)slice * px() * 4;
        f.accum = accum + (size_t)slice * px() * 4;
        return f;
    }
};

// cold / devices: round r renders r + 1 frames of the thread's own poses, each round a larger ray buffer than any
// before; the last round's frames are the output.
struct ColdWorker : Worker {
    vr_tree_t tree;
    std::vector<float> poses;   // [rounds][12]
    int w, h;
    float f;
    int set_device = -1, device_after = -1;
    FrameBuffers fb;
    ColdWorker(vr_tree_t t, std::vector<float> p, int w_, int h_, float f_, int dev) : tree(t), poses(std::move(p)), w(w_), h(h_), f(f_), set_device(dev) {
        rounds = 5;
        finish_in_main = dev >= 0;
    }
    bool prepare() override {
        fb.w = w;
        fb.h = h;
        if (!output(&fb.rgba, "rgba", rounds * fb.px() * 4, set_device < 0)) return false;
        if (!output(&fb.accum, "accum", rounds * fb.px() * 4, set_device < 0)) return false;
        if (set_device >= 0) VR(vr_set_device(set_device));   // the stream and the buffers stay on the tree's device
        return true;
    }
    bool call(int r) override {
        std::vector<VrCamera> cams;
        std::vector<VrFrame> frames;
        for (int i = 0; i <= r; ++i) {
            cams.push_back(camera(&poses[12 * i], w, h, f));
            frames.push_back(fb.frame(i));
        }
        VrRenderOptions opt;
        vr_default_options(&opt);
        VR(vr_render_batch(tree, r + 1, cams.data(), &opt, frames.data(), stream));
        return true;
    }
    bool after() override {
        if (set_device >= 0) HIP(hipGetDevice(&device_after));
        return true;
    }
};

bool run_cold(int n_threads, bool devices) {
    const int id = -1;
    HostTree host;
    load_tree("main", host);
    vr_tree_t tree = nullptr;
    if (devices) VR(vr_set_device(0));
    if (!upload_main(host, &tree)) return false;
    const int w = (int)P("w"), h = (int)P("h");
    const float f = (float)P("f");
    const std::vector<float> poses = read_file<float>("cold_poses.raw", (size_t)n_threads * 5 * 12);
    Workers ws;
    for (int t = 0; t < n_threads; ++t)
        ws.emplace_back(new ColdWorker(tree, std::vector<float>(poses.begin() + t * 60, poses.begin() + (t + 1) * 60), w, h, f,
                                       devices ? t % 2 : -1));
    bool ok = run_workers(ws, devices ? "devices_t" : "cold_t", true);
    if (ok) {
        int kept = 1;
        for (auto& wk : ws) {
            auto* c = static_cast<ColdWorker*>(wk.get());
            if (devices && c->device_after != c->set_device) kept = 0;
        }
        if (devices) printf("devices_kept %d\n", kept);
        uint32_t status = 99;
        if (vr_tree_status(tree, &status, 0) != 0) ok = report(-1, "vr_tree_status", 1, vr_last_error());
        printf("status %u\n", status);
    }
    ws.clear();
    (void)vr_tree_free(tree);
    return ok;
}

// ---- mixed: one thread per family on one tree ------------------------------------------------------------------
struct Scene {
    vr_tree_t tree = nullptr, orig = nullptr, clone = nullptr;
    const HostTree* host = nullptr;
    const HostTree* aux = nullptr;
    int w, h, n_rays, n_points;
    float f, bg, grad_scale;
    std::vector<float> poses, aux_pose, o, d, g, target, points, qdirs;
    std::vector<uint16_t> data_a, data_b;
};

struct RayInputs {
    float *o = nullptr, *d = nullptr;
    VrRays rays() const { return VrRays{o, d}; }
};

struct BatchWorker : Worker {   // vr_render_batch; n_frames frames per round, or one frame per round into slice r
    const Scene& s;
    vr_tree_t tree;
    const std::vector<float>& poses;
    int n_frames;
    bool slices;
    FrameBuffers fb;
    BatchWorker(const Scene& sc, vr_tree_t t, const std::vector<float>& p, int n, bool sl, int n_rounds) : s(sc), tree(t), poses(p), n_frames(n), slices(sl) { rounds = n_rounds; }
    bool prepare() override {
        fb.w = s.w;
        fb.h = s.h;
        const size_t n = slices ? (size_t)rounds : (size_t)n_frames;
        return output(&fb.rgba, "rgba", n * fb.px() * 4, !slices) && output(&fb.accum, "accum", n * fb.px() * 4, !slices);
    }
    bool call(int r) override {
        std::vector<VrCamera> cams;
        std::vector<VrFrame> frames;
        for (int i = 0; i < n_frames; ++i) {
            cams.push_back(camera(&poses[12 * i], s.w, s.h, s.f));
            frames.push_back(fb.frame(slices ? r : i));
        }
        VrRenderOptions opt;
        vr_default_options(&opt);
        VR(vr_render_batch(tree, n_frames, cams.data(), &opt, frames.data(), stream));
        return true;
    }
};

struct AovWorker : Worker {
    const Scene& s;
    FrameBuffers fb;
    float *depth = nullptr, *trans = nullptr;
    explicit AovWorker(const Scene& sc) : s(sc) {}
    bool prepare() override {
        fb.w = s.w;
        fb.h = s.h;
        return output(&fb.rgba, "rgba", 2 * fb.px() * 4, true) && output(&fb.accum, "accum", 2 * fb.px() * 4, true) &&
               output(&depth, "depth", 2 * fb.px(), true) && output(&trans, "trans", 2 * fb.px(), true);
    }
    bool call(int) override {
        VrCamera cams[2];
        VrFrame frames[2];
        VrAov aovs[2];
        for (int i = 0; i < 2; ++i) {
            cams[i] = camera(&s.poses[12 * i], s.w, s.h, s.f);
            frames[i] = fb.frame(i);
            aovs[i] = VrAov{depth + i * fb.px(), trans + i * fb.px(), 0};
        }
        VrRenderOptions opt;
        vr_default_options(&opt);
        VR(vr_render_aov(s.tree, 2, cams, &opt, frames, aovs, VR_DEPTH_TREE, stream));
        return true;
    }
};

struct RaysWorker : Worker {
    const Scene& s;
    RayInputs in;
    uint8_t* rgba = nullptr;
    float* accum = nullptr;
    explicit RaysWorker(const Scene& sc) : s(sc) {}
    bool prepare() override {
        return input(&in.o, s.o) && input(&in.d, s.d) && output(&rgba, "rgba", (size_t)s.n_rays * 4, true) &&
               output(&accum, "accum", (size_t)s.n_rays * 4, true);
    }
    bool call(int) override {
        const VrRays rays = in.rays();
        const VrRayOut out{rgba, accum};
        VrRenderOptions opt;
        vr_default_options(&opt);
        VR(vr_render_rays(s.tree, s.n_rays, &rays, &opt, VR_FP_STRICT, &out, stream));
        return true;
    }
};

struct WeightsWorker : Worker {   // frames (vr_accumulate_weights) or the ray list (vr_accumulate_weights_rays)
    const Scene& s;
    bool list;
    RayInputs in;
    float* mw = nullptr;
    uint32_t* hits = nullptr;
    WeightsWorker(const Scene& sc, bool l) : s(sc), list(l) {}
    bool prepare() override {
        if (list && !(input(&in.o, s.o) && input(&in.d, s.d))) return false;
        return output(&mw, "max_weight", s.host->slots(), false) && output(&hits, "hits", s.host->slots(), false);
    }
    bool call(int) override {
        const VrLeafWeights out{mw, hits};
        VrRenderOptions opt;
        vr_default_options(&opt);
        if (list) {
            const VrRays rays = in.rays();
            VR(vr_accumulate_weights_rays(s.tree, s.n_rays, &rays, &opt, VR_FP_STRICT, &out, stream));
        } else {
            const VrCamera cams[2] = {camera(&s.poses[0], s.w, s.h, s.f), camera(&s.poses[12], s.w, s.h, s.f)};
            VR(vr_accumulate_weights(s.tree, 2, cams, &opt, VR_FP_STRICT, &out, stream));
        }
        return true;
    }
};

struct QueryWorker : Worker {
    const Scene& s;
    float *pts = nullptr, *dirs = nullptr;
    VrQueryOut out{};
    explicit QueryWorker(const Scene& sc) : s(sc) {}
    bool prepare() override {
        const size_t n = (size_t)s.n_points;
        return input(&pts, s.points) && input(&dirs, s.qdirs) && output(&out.sigma, "sigma", n, true) &&
               output(&out.depth, "depth", n, true) && output(&out.coeffs, "coeffs", n * (s.host->d.data_dim - 1), true) &&
               output(&out.rgb, "rgb", n * 3, true);
    }
    bool call(int) override {
        VR(vr_query_points(s.tree, s.n_points, pts, dirs, VR_SPACE_TREE, &out, stream));
        return true;
    }
};

struct OrderWorker : Worker {
    const Scene& s;
    RayInputs in;
    VrRayOrder out{};
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    explicit OrderWorker(const Scene& sc) : s(sc) {}
    bool prepare() override {
        const size_t n = (size_t)s.n_rays;
        workspace_bytes = (size_t)vr_order_rays_workspace(s.n_rays);
        char* ws = nullptr;
        if (!alloc(&ws, workspace_bytes)) return false;
        workspace = ws;
        return input(&in.o, s.o) && input(&in.d, s.d) && output(&out.order, "order", n, true) && output(&out.keys, "keys", n, true) &&
               output(&out.origins_out, "origins", n * 3, true) && output(&out.dirs_out, "dirs", n * 3, true);
    }
    bool call(int) override {
        const VrRays rays = in.rays();
        VrRenderOptions opt;
        vr_default_options(&opt);
        VR(vr_order_rays(s.tree, s.n_rays, &rays, &opt, VR_FP_STRICT, &out, workspace, workspace_bytes, stream));
        return true;
    }
};

struct BackwardWorker : Worker {   // vr_render_backward_rays_touched: every round adds the list's gradient once more
    const Scene& s;
    RayInputs in;
    float *g = nullptr, *grad = nullptr;
    uint32_t* touched = nullptr;
    explicit BackwardWorker(const Scene& sc) : s(sc) {}
    bool prepare() override {
        return input(&in.o, s.o) && input(&in.d, s.d) && input(&g, s.g) && output(&grad, "grad", s.host->elems(), false) &&
               output(&touched, "touched", (s.host->slots() + 31) / 32, false);
    }
    bool call(int) override {
        const VrRays rays = in.rays();
        VrRenderOptions opt;
        vr_default_options(&opt);
        VR(vr_render_backward_rays_touched(s.tree, s.n_rays, &rays, &opt, VR_FP_STRICT, g, grad, touched, stream));
        return true;
    }
};

struct FitWorker : Worker {
    const Scene& s;
    RayInputs in;
    float* target = nullptr;
    VrFit fit{};
    explicit FitWorker(const Scene& sc) : s(sc) {}
    bool prepare() override {
        fit.grad_scale = s.grad_scale;
        if (!(input(&in.o, s.o) && input(&in.d, s.d) && input(&target, s.target))) return false;
        fit.target = target;
        return output(&fit.grad_data, "grad", s.host->elems(), false) && output(&fit.touched, "touched", (s.host->slots() + 31) / 32, false) &&
               output(&fit.sq_err, "sq_err", (size_t)s.n_rays, true) && output(&fit.accum, "accum", (size_t)s.n_rays * 4, true);
    }
    bool call(int) override {
        const VrRays rays = in.rays();
        VrRenderOptions opt;
        vr_default_options(&opt);
        opt.background_brightness = s.bg;
        VR(vr_fit_rays(s.tree, s.n_rays, &rays, &opt, VR_FP_STRICT, &fit, stream));
        return true;
    }
};

// Scheduling knobs that must not change any result, and the tree's synchronous read-outs.
struct TuningWorker : Worker {
    const Scene& s;
    uint32_t status_seen = 0;
    explicit TuningWorker(const Scene& sc) : s(sc) { rounds = 16; }
    bool prepare() override { return true; }
    bool call(int r) override {
        static const int sets[4][3] = {{64, 1, 0}, {0, 64, 64}, {64, 20, 0}, {0, 20, 16}};   // chunk_max, refill_min, drain_flush
        VR(vr_tree_set_tuning(s.tree, "chunk_max", sets[r % 4][0]));
        VR(vr_tree_set_tuning(s.tree, "refill_min", sets[r % 4][1]));
        VR(vr_tree_set_tuning(s.tree, "drain_flush", sets[r % 4][2]));
        uint32_t status = 0;
        uint64_t sched[8], head[3];
        VR(vr_tree_status(s.tree, &status, 0));
        VR(vr_sched_stats(s.tree, sched, 0));
        VR(vr_tree_head_stats(s.tree, head, 0));
        status_seen |= status;
        return true;
    }
};

struct CloneWorker : Worker {   // the clone's values alternate between A and B; one frame behind each update
    const Scene& s;
    uint16_t *a = nullptr, *b = nullptr;
    FrameBuffers fb;
    explicit CloneWorker(const Scene& sc) : s(sc) { rounds = 6; }
    bool prepare() override {
        fb.w = s.w;
        fb.h = s.h;
        return input(&a, s.data_a) && input(&b, s.data_b) && output(&fb.rgba, "rgba", rounds * fb.px() * 4, false) &&
               output(&fb.accum, "accum", rounds * fb.px() * 4, false);
    }
    bool call(int j) override {
        VR(vr_tree_update_data(s.clone, j % 2 ? b : a, VR_DATA_F16, stream));
        const VrCamera cam = camera(s.aux_pose.data(), s.w, s.h, s.f);
        const VrFrame frame = fb.frame(j);
        VrRenderOptions opt;
        vr_default_options(&opt);
        VR(vr_render_batch(s.clone, 1, &cam, &opt, &frame, stream));
        return true;
    }
};

bool run_mixed() {
    const int id = -1;
    HostTree host, aux;
    load_tree("main", host);
    load_tree("aux", aux);
    Scene s;
    s.host = &host;
    s.aux = &aux;
    s.w = (int)P("w");
    s.h = (int)P("h");
    s.f = (float)P("f");
    s.n_rays = (int)P("n_rays");
    s.n_points = (int)P("n_points");
    s.bg = (float)P("bg");
    s.grad_scale = (float)P("grad_scale");
    s.poses = read_file<float>("frame_poses.raw", 24);
    s.aux_pose = read_file<float>("aux_pose.raw", 12);
    s.o = read_file<float>("rays_o.raw", (size_t)s.n_rays * 3);
    s.d = read_file<float>("rays_d.raw", (size_t)s.n_rays * 3);
    s.g = read_file<float>("rays_g.raw", (size_t)s.n_rays * 4);
    s.target = read_file<float>("rays_target.raw", (size_t)s.n_rays * 3);
    s.points = read_file<float>("points.raw", (size_t)s.n_points * 3);
    s.qdirs = read_file<float>("point_dirs.raw", (size_t)s.n_points * 3);
    s.data_a = read_file<uint16_t>("aux_A.data", aux.elems());
    s.data_b = read_file<uint16_t>("aux_B.data", aux.elems());
    bool ok = true;
    for (int pass = 0; pass < 2 && ok; ++pass) {   // the same scripts on fresh trees: serially, then threaded
        if (!upload_main(host, &s.tree)) return false;
        VR(vr_tree_upload(&aux.d, &s.orig));
        VR(vr_tree_clone(s.orig, 0, &s.clone));
        Workers ws;
        ws.emplace_back(new BatchWorker(s, s.tree, s.poses, 2, false, 4));
        ws.emplace_back(new AovWorker(s));
        ws.emplace_back(new RaysWorker(s));
        ws.emplace_back(new WeightsWorker(s, false));
        ws.emplace_back(new WeightsWorker(s, true));
        ws.emplace_back(new QueryWorker(s));
        ws.emplace_back(new OrderWorker(s));
        ws.emplace_back(new BackwardWorker(s));
        ws.emplace_back(new FitWorker(s));
        auto* tuning = new TuningWorker(s);
        ws.emplace_back(tuning);
        ws.emplace_back(new CloneWorker(s));
        ws.emplace_back(new BatchWorker(s, s.orig, s.aux_pose, 1, true, 6));
        const std::string prefix = pass ? "threaded_" : "serial_";
        ok = run_workers(ws, prefix, pass == 1);
        if (ok) {
            uint32_t st[3] = {99, 99, 99};
            vr_tree_t trees[3] = {s.tree, s.orig, s.clone};
            for (int i = 0; i < 3; ++i)
                if (vr_tree_status(trees[i], &st[i], 0) != 0) ok = report(-1, "vr_tree_status", 1, vr_last_error());
            printf("%sstatus %u\n", prefix.c_str(), st[0] | st[1] | st[2] | tuning->status_seen);
        }
        ws.clear();
        (void)vr_tree_free(s.clone);
        (void)vr_tree_free(s.orig);
        (void)vr_tree_free(s.tree);
    }
    return ok;
}

// ---- uploads: four kinds of upload at the same moment, beside two threads that render ----------------------------
struct UploadWorker : Worker {
    enum Kind { kPlain, kQuantised, kDevice, kStaged } kind;
    const HostTree& host;
    std::vector<float> pose;
    int size;
    float f;
    vr_tree_t tree = nullptr;
    FrameBuffers fb;
    uint16_t* read = nullptr;
    int32_t* child_dev = nullptr;
    uint16_t* data_dev = nullptr;
    UploadWorker(Kind k, const HostTree& h, std::vector<float> p, int sz, float f_) : kind(k), host(h), pose(std::move(p)), size(sz), f(f_) { rounds = 1; }
    ~UploadWorker() override {
        if (tree) (void)vr_tree_free(tree);
    }
    bool prepare() override {
        fb.w = fb.h = size;
        if (kind == kDevice && !(input(&child_dev, host.child) && input(&data_dev, host.data))) return false;
        return output(&fb.rgba, "rgba", fb.px() * 4, true) && output(&fb.accum, "accum", fb.px() * 4, true) &&
               output(&read, "data", host.elems(), true);
    }
    bool call(int) override {
        VrTreeDesc d = host.d;
        if (kind == kDevice) {
            d.child = child_dev;
            d.data = data_dev;
            d.memory = 1;
        }
        if (kind == kQuantised) VR(vr_tree_upload_quantized(&d, &host.q, &tree));
        else VR(vr_tree_upload(&d, &tree));
        const VrCamera cam = camera(pose.data(), size, size, f);
        const VrFrame frame = fb.frame(0);
        VrRenderOptions opt;
        vr_default_options(&opt);
        VR(vr_render_batch(tree, 1, &cam, &opt, &frame, stream));
        VR(vr_tree_read_data(tree, read, VR_DATA_F16, stream));
        return true;
    }
    bool after() override {
        HIP(hipStreamSynchronize(stream));
        uint32_t status = 99;
        VR(vr_tree_status(tree, &status, 0));
        if (status != 0) return report(id, "vr_tree_status", (int)status, "status word set");
        return true;
    }
};

bool run_uploads() {
    const int id = -1;
    HostTree host, plain, quant, staged;
    load_tree("main", host);
    load_tree("aux", plain);
    load_tree("quant", quant);
    load_tree("staged", staged);
    Scene s;
    s.host = &host;
    s.w = (int)P("w");
    s.h = (int)P("h");
    s.f = (float)P("f");
    s.poses = read_file<float>("frame_poses.raw", 24);
    const std::vector<float> pose = read_file<float>("upload_pose.raw", 12);
    const int size = (int)P("upload_size");
    const float f = (float)P("upload_f");
    if (!upload_main(host, &s.tree)) return false;
    Workers ws;
    ws.emplace_back(new UploadWorker(UploadWorker::kPlain, plain, pose, size, f));
    ws.emplace_back(new UploadWorker(UploadWorker::kQuantised, quant, pose, size, f));
    ws.emplace_back(new UploadWorker(UploadWorker::kDevice, host, pose, size, f));
    ws.emplace_back(new UploadWorker(UploadWorker::kStaged, staged, pose, size, f));
    const std::vector<float> second(s.poses.begin() + 12, s.poses.end());
    ws.emplace_back(new BatchWorker(s, s.tree, s.poses, 1, true, 8));
    ws.emplace_back(new BatchWorker(s, s.tree, second, 1, true, 8));
    bool ok = run_workers(ws, "uploads_", true);
    if (ok) {
        uint32_t status = 99;
        VR(vr_tree_status(s.tree, &status, 0));
        printf("status %u\n", status);
    }
    ws.clear();
    (void)vr_tree_free(s.tree);
    return ok && !g_stop.load();
}

}  // namespace
#endif  // __HIP_PLATFORM_AMD__

int main(int argc, char* argv[]) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "errors") return run_errors();
#ifdef __HIP_PLATFORM_AMD__
    if (argc < 3) return 2;
    g_dir = argv[2];
    {
        std::ifstream f(g_dir + "/params.txt");
        std::string key;
        double value;
        while (f >> key >> value) g_params[key] = value;
    }
    if (mode == "cold") return run_cold(12, false) ? 0 : 1;
    if (mode == "devices") {
        int count = 0;
        if (vr_device_count(&count) != 0) {
            printf("ERROR vr_device_count: %s\n", vr_last_error());
            return 1;
        }
        if (count < 2) {
            printf("skipped 1\n");
            return 0;
        }
        return run_cold(8, true) ? 0 : 1;
    }
    if (mode == "mixed") return run_mixed() ? 0 : 1;
    if (mode == "uploads") return run_uploads() ? 0 : 1;
#endif
    return 2;
}
