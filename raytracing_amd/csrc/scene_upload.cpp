// scene_upload.cpp -- the scene side of the library: how a scene is uploaded (rt_scene_upload and its stages), how its trees are chosen, folded and
// adapted (OwnTree, choose_tree, FoldAdapt's worker), refitted (rt_scene_refit*; refit_device is also where every pose, skin and morph of scene_moved.cpp
// ends), handed from one context of a group to another (rt_scene_export_folds, rt_scene_import_folds) and inspected (rt_scene_tree_report, the rt_debug_*
// forms of the tree work).  Host code only, on context.h and fold_adapt.h: the tree work on the device goes through devfold::, refit:: and filt::, units of their own, and the three
// things this file needs of the frames' unit are context.h's -- quiesce, relayout_records (the one place it would launch kernels of the hot path's code
// object) and fail.  It touches no frame; the adaptation's render-thread side -- probe, hand-over, adoption -- is frame_fold_hooks.cpp's.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <cmath>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>
#include "rt_hip.h"
#include "context.h"
#include "fold_adapt.h"
#include "own_bvh.h"
#include "treelet_order.h"
#include "tree_select.h"
#include "tree_rotate.h"
#include "wide_bvh.h"        // the host-side fold, the pair layout, the adaptation's host walks (wide_bvh.cpp); wide_node.h: RT_LEAF_BIT, RT_EMPTY_REF
#include "device_fold.h"     // ... and the fold + crossing counts on the device (device_fold.hip)
#include "refit.h"           // the refit of the scene's trees when its triangles move (refit.hip)
#include "filters_host.h"    // filt::snapshot_pose, the pose a refit replaces (filters.hip)
#include "device_memory.h"   // who owns a device allocation: dev::Mem
using namespace rtw;
using namespace context;

// ---- which tree a ray population walks, and the fold adaptation's worker ---------------------------------------------------------------------------
// Everything is in the anonymous namespace but what fold_adapt.h declares for the context's and the frames' units.
namespace
{
// (the host-side fold, the pair layout and the adaptation's host walks: wide_bvh.cpp; the fold on the device: device_fold.hip)
// Which tree a ray population walks: the candidate of own_bvh.h against the reference's own topology (`ref_wide`), both
// walked by proxy rays of that population (tree_select.h).  mode 1: own only if it saves more than 10 % of the steps (the proxy rays are not the
// camera's: a tree that promised 6 % fewer steps on the ShaderBalls-class scene made its shadow trace 10 % slower, profiles/r04_call01_*);
// mode 2: own whatever it costs (A/B runs); mode 3 (shadow): own with the plain surface-area metric, unconditionally (A/B).
struct OwnTree
{
    std::vector<WideNode> wide; uint32_t entry = 0; bool ok = false; const char* name = ""; std::thread worker;
    std::vector<rt_bvh_node> bvh2; std::vector<uint32_t> roots;    // the binary tree the records fold, and the node each record tests (FoldAdapt)
    dev::Mem d_wide;                                               // the records on the device already (RT_CTX_OPT_DEVICE_FOLD); whoever adopts them owns them
    int device = -1;                                               // >= 0: fold on that device (a stream of the worker's own)
    bool pairs = false;                                            // RT_CTX_OPT_WIDE_LAYOUT
    bool device_builder = false;                                   // RT_CTX_OPT_TREE_BUILDER: the binary tree itself is built on the device (PLOC, ploc_kernels.h) ...
    bool device_only = false;                                      // ... and if that fails this candidate is simply not there (another OwnTree is the host-built candidate)
    std::atomic<bool> cancel_build{false};                         // the host build gives up: another candidate has won
    bool built_on_device = false; uint32_t ploc_rounds = 0;
    // RT_CTX_OPT_TREE_BUILDER = 1: tree AND fold on the device -- the reference's nodes go up once, the tree is clustered there (devfold::build_tree), folded there
    // (devfold::fold takes the device array as it is) and comes back once for the adaptation's host side; false = something failed: the host path takes over
    bool build_and_fold_on_device(const rt_scene_desc* sd, const ownbvh::Metric& m)
    {
        if (device < 0 || hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return false; }
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return false; }
        dev::Mem d_ref, d_tree;                                    // the reference's nodes and the tree built from them: freed on the way out, the stream waited for
        rt_bvh_node* tree = nullptr;
        WideNode* recs = nullptr;
        uint32_t n_tree = 0, n = 0;
        const size_t ref_bytes = (size_t)sd->num_nodes * sizeof(rt_bvh_node);
        bool done = d_ref.alloc(ref_bytes) && d_ref.upload(st, sd->nodes, ref_bytes);
        const auto t0 = std::chrono::steady_clock::now();
        done = done && devfold::build_tree(st, d_ref.get<const rt_bvh_node>(), sd->num_nodes, sd->nodes[0], &m, &tree, &n_tree, &bvh2, nullptr, nullptr, &ploc_rounds);
        d_tree = dev::Mem(tree);
        build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const auto t1 = std::chrono::steady_clock::now();
        done = done && devfold::fold(st, tree, n_tree, bvh2[0], &m, nullptr, &recs, &n, &entry, &roots, &wide) && n != 0u;
        d_wide = dev::Mem(recs);
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
        (void)hipGetLastError();
        if (!done) { d_wide.free(); bvh2.clear(); wide.clear(); roots.clear(); return false; }
        if (pairs)
        {
            pair_layout_by_area(wide, roots, bvh2.data(), (uint32_t)bvh2.size(), &m);
            if (hipMemcpy(d_wide.get(), wide.data(), wide.size() * sizeof(WideNode), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); d_wide.free(); return false; }
        }
        fold_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        built_on_device = true;
        name = name_device.c_str();
        return true;
    }
    std::string name_device;
    double fold_seconds = 0.0, build_seconds = 0.0;
    // the collapse of the finished binary tree: on the device (the tree goes up, the records stay there and come back for the choice by proxy rays), or by build_wide_bvh
    bool fold_it(const ownbvh::Metric& m)
    {
        const auto t0 = std::chrono::steady_clock::now();
        bool done = false;
        if (device >= 0 && hipSetDevice(device) == hipSuccess)
        {
            hipStream_t st = nullptr;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess)
            {
                dev::Mem d_nodes;                                  // (freed at the end of this block: the stream has been waited for)
                const size_t bytes = bvh2.size() * sizeof(rt_bvh_node);
                if (d_nodes.alloc(bytes) && d_nodes.upload(st, bvh2.data(), bytes))
                {
                    uint32_t n = 0;
                    WideNode* recs = nullptr;
                    done = devfold::fold(st, d_nodes.get<const rt_bvh_node>(), (uint32_t)bvh2.size(), bvh2[0], &m, nullptr, &recs, &n, &entry, &roots, &wide) && n != 0u;
                    d_wide = dev::Mem(recs);
                }
                (void)hipStreamSynchronize(st);
                (void)hipStreamDestroy(st);
            }
            (void)hipGetLastError();
            if (!done) d_wide.free();
        }
        if (!done) done = build_wide_bvh(bvh2.data(), (uint32_t)bvh2.size(), RT_WIDE_SAH, wide, entry, &roots, &m) && !wide.empty();
        if (done && pairs)
        {
            pair_layout_by_area(wide, roots, bvh2.data(), (uint32_t)bvh2.size(), &m);
            if (d_wide && hipMemcpy(d_wide.get(), wide.data(), wide.size() * sizeof(WideNode), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); d_wide.free(); }
        }
        fold_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return done;
    }
    void start(const rt_scene_desc* sd, bool shadow, uint32_t mode)
    {
        ownbvh::Metric m;
        name = "own: surface area";
        if (shadow && mode != 3u)
        {
            ownbvh::Metric d = shadow_metric(sd->lights, sd->num_lights, 0.5);
            if (!d.dirs.empty()) { m = d; name = "own: projected area along the directional lights + 50 % isotropic"; }
        }
        name_device = std::string(name) + ", built on the device (PLOC)";
        worker = std::thread([this, sd, m]()
        {
            if (device_builder && build_and_fold_on_device(sd, m)) { ok = true; return; }
            if (device_only) { ok = false; return; }
            const auto t0 = std::chrono::steady_clock::now();
            ok = ownbvh::build(sd->nodes, sd->num_nodes, m, bvh2, &cancel_build);
            build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            ok = ok && fold_it(m);
        });
    }
    void join() { if (worker.joinable()) worker.join(); }
    ~OwnTree() { join(); }
};

// What every candidate of one ray population is measured against and with: the proxy rays (an area-weighted pass over all triangles), the leaf of every first
// triangle, the reference fold's cost -- made by the first choose_tree call and kept for the next (the device-built candidate, then the host-built one).
struct ChoiceInputs
{
    bool valid = false;
    std::vector<uint32_t> leaf_of_first;
    std::vector<treesel::ProxyRay> rays;
    double c_ref = 0.0;
};

// true: walk the own tree; false: keep the reference topology
bool choose_tree(const rt_scene_desc* sd, const std::vector<WideNode>& ref_wide, uint32_t ref_entry, bool shadow, uint32_t mode,
    OwnTree& own, std::string& report, ChoiceInputs* kept = nullptr)
{
    own.join();
    char line[320];
    if (!own.ok) { report += shadow ? "shadow tree: the own tree does not qualify -> reference topology\n" : "closest-hit tree: the own tree does not qualify -> reference topology\n"; return false; }
    if (mode >= 2u)
    {
        snprintf(line, sizeof(line), "%s tree: %s, forced (not measured)\n", shadow ? "shadow" : "closest-hit", own.name);
        report += line;
        return true;
    }
    const uint32_t nt = sd->num_triangles, nn = sd->num_nodes;
    ChoiceInputs mine;
    ChoiceInputs& in = kept ? *kept : mine;
    if (!in.valid)
    {
        in.leaf_of_first.assign(nt, 0u);
        for (uint32_t i = 0; i < nn; ++i)
            if ((sd->nodes[i].num_primitives_axis >> 16) != 0 && sd->nodes[i].offset < nt) in.leaf_of_first[sd->nodes[i].offset] = i;
        in.rays = treesel::proxy_rays(sd->triangles, nt, sd->lights, sd->num_lights, 8192u, shadow);
        if (!in.rays.empty())
            in.c_ref = treesel::walk_cost((const treesel::Record*)ref_wide.data(), (uint32_t)ref_wide.size(), ref_entry, sd->nodes, in.leaf_of_first.data(), sd->triangles, in.rays, shadow);
        in.valid = true;
    }
    const std::vector<uint32_t>& leaf_of_first = in.leaf_of_first;
    const std::vector<treesel::ProxyRay>& rays = in.rays;
    if (rays.empty()) { report += shadow ? "shadow tree: no lights, nothing to measure -> reference topology\n" : "closest-hit tree: nothing to measure -> reference topology\n"; return false; }
    const double c_ref = in.c_ref;
    const double c_own = treesel::walk_cost((const treesel::Record*)own.wide.data(), (uint32_t)own.wide.size(), own.entry, sd->nodes, leaf_of_first.data(), sd->triangles, rays, shadow);
    const bool pick = c_own < 0.90 * c_ref;
    snprintf(line, sizeof(line), "%s tree: reference topology %.2f steps per proxy ray, %s %.2f -> %s\n", shadow ? "shadow" : "closest-hit", c_ref, own.name, c_own,
        pick ? "own" : "reference topology");
    report += line;
    return pick;
}

} // namespace

// ---- Fold adaptation (RT_CTX_OPT_ADAPTIVE_FOLD): FoldAdapt is fold_adapt.h's; what follows is its worker's side ------------------------------------
namespace context
{
void drop_fold_adapt(FoldAdapt* a) { delete a; }
void fold_adapt_set_interval(FoldAdapt* a, uint32_t ms) { a->min_interval_ms = ms; }
void fold_adapt_set_wait(FoldAdapt* a, bool wait) { if (wait) a->mode.fetch_or(2u); else a->mode.fetch_and(~2u); }
} // namespace context

namespace
{

// One tree folded again for the rays that were counted on it.  cost[] = what the current and the new fold cost those rays.
// fold_device >= 0 (RT_CTX_OPT_DEVICE_FOLD): the crossing counts and the collapse run on that device, on a stream of the calling (worker) thread's own -- the tree
// goes up once per call (the shadow rays' tree changes with every rotation), the records come back for the host's bookkeeping; anything that fails there
// is done here on host threads instead.
bool refold_for_rays(const std::vector<rt_bvh_node>& tree, const std::vector<float4>& o, const std::vector<float4>& d, const std::vector<uint32_t>& roots_now,
    std::vector<WideNode>& out, uint32_t& entry, double (&cost)[2], const std::atomic<bool>& cancel, std::vector<uint32_t>* roots_out = nullptr, int fold_device = -1,
    bool pairs = false /* RT_CTX_OPT_WIDE_LAYOUT: the new records in (parent, likeliest child) pairs, by the measured weights */)
{
    if (tree.empty() || o.empty() || o.size() != d.size() || roots_now.empty()) return false;
    const uint32_t nn = (uint32_t)tree.size();
    std::vector<uint32_t> counts;
    struct DeviceTree
    {
        hipStream_t st = nullptr; dev::Mem nodes;                  // (nodes is freed after this destructor has waited for the stream)
        ~DeviceTree() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } (void)hipGetLastError(); }
    } dt;
    bool on_device = false;
    if (fold_device >= 0 && hipSetDevice(fold_device) == hipSuccess && hipStreamCreateWithFlags(&dt.st, hipStreamNonBlocking) == hipSuccess)
    {
        on_device = dt.nodes.alloc((size_t)nn * sizeof(rt_bvh_node)) && dt.nodes.upload(dt.st, tree.data(), (size_t)nn * sizeof(rt_bvh_node));
        if (on_device)
        {
            uint64_t truncated = 0;
            on_device = devfold::count_box_passes(dt.st, dt.nodes.get<const rt_bvh_node>(), nn, o.data(), d.data(), o.size(), counts, &truncated);
            if (truncated) truncated_walks_add(truncated);
        }
        if (!on_device) (void)hipGetLastError();
    }
    if (!on_device) count_box_passes(tree.data(), nn, o.data(), d.data(), o.size(), counts, cancel);
    if (cancel.load()) return false;
    // the measured passes, plus a twentieth of their sum spread by surface area: boxes no probe ray met still fold sensibly
    std::vector<double> w(nn);
    double total = 0.0, area_sum = 0.0;
    {
        // (64 slices whatever the host, taken by up to 16 threads, their partial sums added in slice order: 4.9 M nodes on the headline scene, twice per adaptation)
        const unsigned K = nn >= 262144u ? 64u : 1u, T = K > 1u ? adapt_threads(nn, 131072) : 1u;
        std::vector<double> part_total(K, 0.0), part_area(K, 0.0);
        auto slice = [&](unsigned k, int pass, double prior)
        {
            double tt = 0.0, aa = 0.0;
            for (uint32_t n = (uint32_t)((uint64_t)nn * k / K), e = (uint32_t)((uint64_t)nn * (k + 1) / K); n < e; ++n)
            {
                if (pass == 1) { w[n] = (double)counts[n] + prior * w[n]; continue; }
                const rt_bvh_node& b = tree[n];
                const double dx = (double)b.bounds_max.x - b.bounds_min.x, dy = (double)b.bounds_max.y - b.bounds_min.y, dz = (double)b.bounds_max.z - b.bounds_min.z;
                w[n] = dx * dy + dy * dz + dz * dx;
                aa += w[n];
                tt += (double)counts[n];
            }
            if (pass == 0) { part_total[k] = tt; part_area[k] = aa; }
        };
        auto on_slices = [&](int pass, double prior)
        {
            std::atomic<unsigned> next{0};
            auto run = [&]() { for (unsigned k; (k = next.fetch_add(1)) < K;) slice(k, pass, prior); };
            std::vector<std::thread> pool;
            for (unsigned t = 1; t < T; ++t) pool.emplace_back(run);
            run();
            for (auto& th : pool) th.join();
        };
        on_slices(0, 0.0);
        for (unsigned k = 0; k < K; ++k) { total += part_total[k]; area_sum += part_area[k]; }
        if (!(total > 0.0) || !(area_sum > 0.0) || !std::isfinite(area_sum)) return false;
        on_slices(1, 0.05 * total / area_sum);
    }
    // what the fold on the device costs these rays: known before, and whether or not, a new fold can be built (a failed build
    // used to leave it 0, and a rotated candidate was then adopted without ever having been compared with it)
    cost[0] = cost[1] = 0.0;
    for (uint32_t r : roots_now) if (r < nn) cost[0] += w[r];
    cost[0] /= (double)o.size();
    std::vector<uint32_t> roots_new;
    bool folded = false;
    if (on_device)
    {
        WideNode* d_recs = nullptr;
        uint32_t n_recs = 0;
        folded = devfold::fold(dt.st, dt.nodes.get<const rt_bvh_node>(), nn, tree[0], nullptr, w.data(), &d_recs, &n_recs, &entry, &roots_new, &out, &cancel) && !out.empty();
        dev::drop(d_recs);                                                 // (the records travel with fold_upload, with the shadow side's slot order applied)
        (void)hipGetLastError();
        if (cancel.load()) return false;
    }
    if (!folded && (!build_wide_bvh(tree.data(), nn, RT_WIDE_SAH, out, entry, &roots_new, nullptr, w.data(), &cancel) || out.empty())) return false;
    for (uint32_t r : roots_new) cost[1] += w[r];
    cost[1] /= (double)o.size();
    if (pairs && roots_new.size() == out.size())
    {
        pair_layout_by_node_weights(out, roots_new, w.data(), nn);
    }
    if (roots_out) roots_out->swap(roots_new);
    return cost[1] < cost[0];
}

// The shadow rays' side of an adaptation.  Their verdict does not depend on the tree above the reference's leaves (own_bvh.h), so with mode bit 3
// the binary tree itself is first rotated for the probe rays' measured crossings (tree_rotate.h) and then folded; whichever of the two folds --
// of the tree as it was, of the rotated tree -- costs the probe rays less is the candidate.
bool adapt_shadow_candidate(FoldAdapt* a)
{
    const std::vector<rt_bvh_node>& tree = a->bvh2_sh.empty() ? a->bvh2 : a->bvh2_sh;
    const std::vector<uint32_t>& roots = a->roots_sh.empty() ? a->roots : a->roots_sh;
    a->rotations = 0;
    a->bvh2_sh_new.clear();
    const int fold_device = a->worker_fold_device();
    auto t_stage = std::chrono::steady_clock::now();
    auto stage = [&](int k) { const auto t = std::chrono::steady_clock::now(); a->stage_s[k] = std::chrono::duration<double>(t - t_stage).count(); t_stage = t; };
    // the fold of the tree as it is and the rotations do not need each other: they run side by side (with the folds on the device -- bit 1 -- and on host threads alike:
    // beside an orbiting camera's frames the adapted fold then lands after 0.56 - 0.62 s instead of 0.69 - 0.74 and the frames cost the same, profiles/r06/call26*.log)
    bool ok = false;
    const bool rotating = (a->mode.load() & 8u) && !a->sh_o.empty();
    std::thread plain_thread;
    auto plain_fold = [&, t0 = t_stage]()
    {
        ok = refold_for_rays(tree, a->sh_o, a->sh_d, roots, a->wide_sh, a->entry_sh, a->cost[1], a->cancel, &a->roots_sh_new, fold_device, a->pairs);
        a->stage_s[2] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    if (rotating) plain_thread = std::thread(plain_fold); else plain_fold();
    if (!rotating || a->cancel.load()) { if (plain_thread.joinable()) plain_thread.join(); return ok; }
    std::vector<rt_bvh_node> rotated;
    double crossings[2] = {0.0, 0.0};
    const uint32_t made = treerot::rotate(tree.data(), (uint32_t)tree.size(), (const float*)a->sh_o.data(), (const float*)a->sh_d.data(), a->sh_o.size(), 8, rotated, crossings, &a->cancel, 3, 0.03, a->rotate_s);
    stage(3);
    if (plain_thread.joinable()) plain_thread.join();
    if (made == 0 || rotated.size() != tree.size() || a->cancel.load()) return ok;
    std::vector<WideNode> wide;
    std::vector<uint32_t> roots_rot;
    uint32_t entry = 0;
    double cost[2] = {0.0, 0.0};
    const std::vector<uint32_t> top{0u};                                   // (the rotated tree has no current fold: only cost[1] is read)
    (void)refold_for_rays(rotated, a->sh_o, a->sh_d, top, wide, entry, cost, a->cancel, &roots_rot, fold_device, a->pairs);
    stage(4);
    if (wide.empty() || roots_rot.empty() || a->cancel.load()) return ok;
    // the rotated tree's boxes differ, so its measured passes are compared as they are (both are box passes per probe ray at record roots);
    // without a known cost of the fold on the device nothing is adopted
    if (!(a->cost[1][0] > 0.0)) return ok;
    const double current = a->cost[1][0], plain = ok ? a->cost[1][1] : current;
    if (!(cost[1] < plain)) return ok;
    a->wide_sh.swap(wide); a->entry_sh = entry; a->roots_sh_new.swap(roots_rot); a->bvh2_sh_new.swap(rotated);
    a->cost[1][1] = cost[1];
    a->rotations = made;
    return cost[1] < current;
}

bool adapt_shadow_side(FoldAdapt* a)
{
    a->reordered = 0;
    // mode bit 4 needs every probe shadow ray's nearest occluder: a walk of the reference's tree that depends on neither the rotations nor the folds, so -- when the
    // folds are the device's and the host's threads are this worker's (bit 1) -- it runs beside them
    const bool want_order = (a->mode.load() & 16u) && !a->tri9.empty() && !a->sh_o.empty();
    std::vector<uint32_t> prim;
    double t_occ = 0.0;
    auto find_occluders = [&]()
    {
        const auto t0 = std::chrono::steady_clock::now();
        nearest_occluders(a->bvh2, a->tri9, a->sh_o, a->sh_d, prim, a->cancel);
        t_occ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    std::thread beside;
    if (want_order && a->worker_fold_device() >= 0) beside = std::thread(find_occluders);
    const bool ok = adapt_shadow_candidate(a);
    if (beside.joinable()) beside.join();
    if (ok && want_order && !a->wide_sh.empty() && !a->cancel.load())
    {
        // the candidate's slots, likeliest occluder first
        const auto t0 = std::chrono::steady_clock::now();
        if (prim.size() != a->sh_o.size()) find_occluders();
        const std::vector<rt_bvh_node>& tree = a->rotations != 0 ? a->bvh2_sh_new : (a->bvh2_sh.empty() ? a->bvh2 : a->bvh2_sh);
        if (!a->cancel.load()) a->reordered = occluder_first(a->wide_sh, a->roots_sh_new, tree, prim);
        a->stage_s[5] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    (void)t_occ;
    return ok;
}

// The probe's queues, as the asynchronous copies left them in the pinned staging area, become the rays the folds are made for
// (closest-hit rays clipped at their hit: a ray that hit something never visits what lies behind the hit).
void probe_unpack(FoldAdapt* a)
{
    if (!a->staging || a->probe_paths == 0) return;                    // rays given directly (rt_debug_fold_abandon)
    a->o.clear(); a->d.clear(); a->sh_o.clear(); a->sh_d.clear();
    for (uint32_t sample = 0; sample < a->probe_samples; ++sample)
    {
        DCounters h;
        memcpy(&h, a->staging + a->probe_counters(sample), sizeof(h));
        for (uint32_t bounce = 0; bounce < a->probe_bounces; ++bounce)
        {
            const uint32_t n = h.queue[bounce], ns = h.shadow[bounce];
            if (n > a->probe_paths || ns > a->probe_paths) { a->o.clear(); a->d.clear(); a->sh_o.clear(); a->sh_d.clear(); return; }
            if (n == 0) break;
            const float4* o = (const float4*)(a->staging + a->probe_block(sample, bounce, 0));
            const float4* d = (const float4*)(a->staging + a->probe_block(sample, bounce, 1));
            const float4* hits = (const float4*)(a->staging + a->probe_block(sample, bounce, 2));
            const size_t at = a->o.size();
            a->o.insert(a->o.end(), o, o + n);
            a->d.insert(a->d.end(), d, d + n);
            for (uint32_t i = 0; i < n; ++i)
            {
                uint32_t prim;
                memcpy(&prim, &hits[i].z, 4);
                if (prim != RT_INVALID_ID && hits[i].w > 0.0f && hits[i].w * 1.0001f < a->o[at + i].w) a->o[at + i].w = hits[i].w * 1.0001f;
            }
            if (ns != 0)
            {
                const float4* so = (const float4*)(a->staging + a->probe_block(sample, bounce, 3));
                const float4* sd = (const float4*)(a->staging + a->probe_block(sample, bounce, 4));
                a->sh_o.insert(a->sh_o.end(), so, so + ns);
                a->sh_d.insert(a->sh_d.end(), sd, sd + ns);
            }
        }
    }
}

// The adapted records go to the device from HERE, on a stream of the worker's own; what earlier adoptions replaced is freed here too, after
// a device synchronisation that only this thread waits for.
void fold_upload(FoldAdapt* a)
{
    if (a->device < 0 || a->cancel.load() || !(a->ok || a->ok_sh)) return;
    a->upload_failed = true;
    if (hipSetDevice(a->device) != hipSuccess) return;
    if (!a->retired.empty())
    {
        if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return; }
        for (void* p : a->retired) (void)hipFree(p);
        a->retired.clear();
    }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return; }
    bool ok = true;
    if (a->ok) ok = hipMalloc(&a->new_cl, a->wide.size() * sizeof(WideNode)) == hipSuccess &&
                    hipMemcpyAsync(a->new_cl, a->wide.data(), a->wide.size() * sizeof(WideNode), hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok && a->ok_sh) ok = hipMalloc(&a->new_sh, a->wide_sh.size() * sizeof(WideNode)) == hipSuccess &&
                             hipMemcpyAsync(a->new_sh, a->wide_sh.data(), a->wide_sh.size() * sizeof(WideNode), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    (void)hipStreamDestroy(st);
    if (!ok)
    {
        (void)hipGetLastError();
        if (a->new_cl) (void)hipFree(a->new_cl);
        if (a->new_sh) (void)hipFree(a->new_sh);
        a->new_cl = a->new_sh = nullptr;
        return;
    }
    a->upload_failed = false;
}
} // namespace

void context::fold_adapt_worker(FoldAdapt* a)
{
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    for (double& t : a->stage_s) t = 0.0;
    probe_unpack(a);
    a->stage_s[0] = since();
    if (!a->o.empty())
    {
        std::thread shadow([a]() { a->ok_sh = adapt_shadow_side(a); });
        a->ok = refold_for_rays(a->bvh2, a->o, a->d, a->roots, a->wide, a->entry, a->cost[0], a->cancel, &a->roots_new, a->worker_fold_device(), a->pairs);
        a->stage_s[1] = since() - a->stage_s[0];
        shadow.join();
        const double t_up = since();
        fold_upload(a);
        a->stage_s[6] = since() - t_up;
    }
    a->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    a->finished.store(true);
}

context::FoldAdapt::~FoldAdapt()
{
    cancel.store(true);
    if (worker.joinable()) worker.join();
    if (device >= 0)
    {
        // (the callers -- rt_scene_upload, rt_ctx_destroy -- free the scene's own records the same way: after their stream synchronisation)
        (void)hipSetDevice(device);
        if (probe_done) { (void)hipEventSynchronize(probe_done); (void)hipEventDestroy(probe_done); }
        if (probe) (void)rt_frame_destroy(probe);
        if (staging) (void)hipHostFree(staging);
        for (void* p : {new_cl, new_sh}) if (p) (void)hipFree(p);
        if (!retired.empty()) (void)hipDeviceSynchronize();
        for (void* p : retired) (void)hipFree(p);
    }
}

// Has the camera left the view the folds were adapted to?  (tools/fold_weight_study.py --views: a fold adapted to one view costs another view
// 0 .. + 2 % against the surface-area fold as a rule and up to + 11 % -- street level seen with a fold made from above -- while its own view
// gains 2 .. 14 %.)  Position by 3 % of the scene's diagonal, direction by 20 degrees, field of view by a tenth.
bool context::fold_view_left(const FoldAdapt& a, const rt_camera& c)
{
    const double dx = (double)c.position.x - a.camera.position.x, dy = (double)c.position.y - a.camera.position.y, dz = (double)c.position.z - a.camera.position.z;
    if (std::sqrt(dx * dx + dy * dy + dz * dz) > 0.03 * a.scene_diagonal) return true;
    const double la = std::sqrt((double)a.camera.front.x * a.camera.front.x + (double)a.camera.front.y * a.camera.front.y + (double)a.camera.front.z * a.camera.front.z);
    const double lc = std::sqrt((double)c.front.x * c.front.x + (double)c.front.y * c.front.y + (double)c.front.z * c.front.z);
    const double dot = (double)c.front.x * a.camera.front.x + (double)c.front.y * a.camera.front.y + (double)c.front.z * a.camera.front.z;
    if (la > 0.0 && lc > 0.0 && !(dot >= 0.9396926 * la * lc)) return true;
    return std::fabs((double)c.fov - a.camera.fov) > 0.1 * std::fabs((double)a.camera.fov);
}

// ---- rt_scene_upload ---------------------------------------------------------------------------------------------------------------------------------
void context::free_scene(Scene& s)
{
    void* ptrs[] = {s.nodes, s.tris_rt, s.tris_sh, s.materials, s.textures, s.texture_data, s.lights, s.env, s.emissive, s.trees[TREE_REF].recs, s.mat_tex16,
        s.trees[TREE_SHADOW].recs, s.trees[TREE_CLOSEST].recs};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (s.adapt) drop_fold_adapt(s.adapt);
    if (s.refit) { refit::release(*s.refit); delete s.refit; }
    if (s.pose_snap) (void)hipFree(s.pose_snap);
    if (s.pose) { pose::release(*s.pose); delete s.pose; }
    if (s.skin) { skin::release(*s.skin); delete s.skin; }
    if (s.morph) { morph::release(*s.morph); delete s.morph; }
    delete s.leaf_starts;
    s = Scene();
}

// The tree report keeps one entry of a kind, the latest: what begins at the first `prefix` goes, `line` is appended.
void context::replace_report_line(std::string& report, const char* prefix, const std::string& line)
{
    const size_t at = report.find(prefix);
    if (at != std::string::npos) report.erase(at);
    report += line;
}

namespace
{

// ---- rt_scene_upload's stages ------------------------------------------------------------------------------------------------------
// do this many 64-byte records stay below 4 GiB?  (k_trace_w4 and k_trace2 address node and trace-triangle records with 32-bit byte offsets)
bool fits_offsets32(uint64_t records) { return records * 64 <= 0xFFFFFFFFull; }

// RT_CTX_OPT_ADAPTIVE_FOLD: is a scene of nn nodes one that gets a fold adaptation?  (bit 0: the option; bit 2: also scenes too small to profit)
bool adaptation_wanted(const rt_ctx* ctx, uint32_t nn) { return (ctx->adaptive_fold & 1u) && (nn >= 8192u || (ctx->adaptive_fold & 4u)); }

// the triangles' corner positions, 9 floats each (FoldAdapt::tri9)
void copy_corners(const rt_triangle* tris, uint32_t nt, std::vector<float>& tri9)
{
    tri9.resize((size_t)nt * 9);
    for (uint32_t i = 0; i < nt; ++i)
    {
        const rt_triangle& t = tris[i];
        const rt_float3 v[3] = {t.v1.position, t.v2.position, t.v3.position};
        for (int k = 0; k < 3; ++k) { tri9[(size_t)i * 9 + 3 * k] = v[k].x; tri9[(size_t)i * 9 + 3 * k + 1] = v[k].y; tri9[(size_t)i * 9 + 3 * k + 2] = v[k].z; }
    }
}

// What an upload has worker threads do beside its own work: the candidate trees of the backend's own (Upload::choose_own_trees) and the copies an adaptation
// keeps of the caller's arrays (FoldAdapt: the binary tree, the triangles' corners -- 157 + 100 MB for 2.8 M triangles).  An upload that ends early
// gives the host builds up before it joins them.
struct UploadWorkers
{
    OwnTree own_sh, own_cl, own_sh_dev;      // own_sh_dev: the shadow rays' candidate built on the device (RT_CTX_OPT_TREE_BUILDER != 0)
    std::vector<rt_bvh_node> bvh2; std::vector<float> tri9; std::thread copies;
    void cancel() { own_sh.cancel_build.store(true); own_cl.cancel_build.store(true); }
    void join_copies() { if (copies.joinable()) copies.join(); }
    ~UploadWorkers() { cancel(); join_copies(); }          // (~OwnTree joins)
};

// One rt_scene_upload: the scene in the making and what its stages hand to each other.  The scene is the context's only once publish() has run; an upload
// that is refused or fails before that frees with this object whatever the stages had allocated, so the context is left without a scene.
struct Upload
{
    rt_ctx* const ctx; const rt_scene_desc* const sd; const uint32_t nt, nn;
    Scene s;
    UploadWorkers w;
    int rc = RT_OK;                           // device allocations and copies that failed so far (looked at once, after the trees are chosen)
    bool may_own = false, try_device_tree = false;
    std::vector<uint32_t> interior_index; uint32_t n_interior = 0;
    std::vector<float4> super_root, lights;   // host staging (like interior_index and wide): read by copies on the stream until the upload's last synchronisation
    std::vector<WideNode> wide; std::vector<uint32_t> wide_roots;   // the fold of the reference's tree on the host; the binary-tree node each of its records tests
    uint32_t w_entry = 0, n_wide_dev = 0, n_wide_ref = 0;
    bool folded_on_device = false, have_wide = false, have_sh = false, have_cl = false;
    OwnTree* sh = nullptr;                    // the shadow rays' candidate that was measured last (the one adopted, if one is)
    std::chrono::steady_clock::time_point t_upload, t_lap;
    double t_layout = 0.0, t_device = 0.0, t_dev_fold = 0.0, t_fold = 0.0, t_own_wait = 0.0, t_choose = 0.0;

    Upload(rt_ctx* c, const rt_scene_desc* d) : ctx(c), sd(d), nt(d->num_triangles), nn(d->num_nodes), t_upload(std::chrono::steady_clock::now()), t_lap(t_upload) {}
    ~Upload() { w.cancel(); free_scene(s); }
    double lap() { const auto n = std::chrono::steady_clock::now(); const double d = std::chrono::duration<double>(n - t_lap).count(); t_lap = n; return d; }

    // the trees of the backend's own (below, "Trees of the backend's own") are built on worker threads meanwhile
    void start_workers()
    {
        OwnTree &own_sh = w.own_sh, &own_cl = w.own_cl, &own_sh_dev = w.own_sh_dev;
        may_own = ctx->build_wide == 1u && fits_offsets32(nt) && (sd->nodes[0].num_primitives_axis >> 16) == 0;
        if (ctx->device_fold && ctx->build_wide == 1u) { own_sh.device = ctx->device; own_cl.device = ctx->device; }
        own_sh.pairs = own_cl.pairs = ctx->wide_layout != 0u;
        // (the shadow rays' tree only: the closest-hit rays' own tree is the tolerance mode's, host-built)
        try_device_tree = may_own && ctx->shadow_tree && ctx->tree_builder != 0u && ctx->device_fold != 0u && ctx->build_wide == 1u;
        if (try_device_tree)
        {
            own_sh_dev.device = ctx->device; own_sh_dev.pairs = own_sh.pairs; own_sh_dev.device_builder = true; own_sh_dev.device_only = true;
            own_sh_dev.start(sd, true, ctx->shadow_tree);
        }
        if (may_own && ctx->shadow_tree && !(try_device_tree && ctx->tree_builder == 1u)) own_sh.start(sd, true, ctx->shadow_tree);
        if (may_own && ctx->closest_tree) own_cl.start(sd, false, ctx->closest_tree);
        // what an adaptation keeps of the caller's arrays is copied beside everything else instead of after it
        if (adaptation_wanted(ctx, nn) && ctx->build_wide == 1u && !ctx->closest_tree)
            w.copies = std::thread([this, corners = (ctx->adaptive_fold & 16u) != 0u]()
            {
                w.bvh2.assign(sd->nodes, sd->nodes + nn);
                if (corners) copy_corners(sd->triangles, nt, w.tri9);
            });
    }

    // BVH re-layout, the host's part: LinearBVHNode[] (bvh.cpp:223-245) -> child-pair records, in treelet order (treelet_order.h: a pure permutation of records;
    // the records themselves are written on the device, relayout_on_device), and the super-root record
    int order_records()
    {
        const int bad = treelet::order(sd->nodes, nn, ctx->treelet_nodes, interior_index, n_interior);
        if (bad == 1) return fail(ctx, "rt_scene_upload: child index outside the node array");
        if (bad != 0) return fail(ctx, "rt_scene_upload: the node array is not a tree (cycle)");
        t_layout = lap();
        const rt_bvh_node& root = sd->nodes[0];
        s.d.root_ref = (root.num_primitives_axis >> 16) > 0 ? (RT_LEAF_BIT | root.offset) : 0u;
        // super-root: child 0 = (root box, root ref), child 1 = empty.  Visiting it IS the
        // reference's first loop iteration (box test of node 0, trace_bvh.cl:146-148).
        s.d.entry_ref = n_interior;
        super_root.resize(4);
        float4* out = super_root.data();
        out[0] = make_float4(root.bounds_min.x, root.bounds_min.y, root.bounds_max.x, root.bounds_max.y);
        out[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[2] = make_float4(root.bounds_min.z, root.bounds_max.z, 0.0f, 0.0f);
        uint32_t r0 = s.d.root_ref, r1 = RT_EMPTY_REF, axis = 0;
        float fr0, fr1, fax;
        memcpy(&fr0, &r0, 4); memcpy(&fr1, &r1, 4); memcpy(&fax, &axis, 4);
        out[3] = make_float4(fr0, fr1, fax, 0.0f);
        s.d.root_min[0] = root.bounds_min.x; s.d.root_min[1] = root.bounds_min.y; s.d.root_min[2] = root.bounds_min.z;
        s.d.root_max[0] = root.bounds_max.x; s.d.root_max[1] = root.bounds_max.y; s.d.root_max[2] = root.bounds_max.z;
        return RT_OK;
    }

    // the lights as the kernels read them, and whether their shadow rays are the slow kind
    void stage_lights()
    {
        lights.resize((size_t)(sd->num_lights ? sd->num_lights : 1) * 3);
        uint32_t slow_lights = 0;
        for (uint32_t i = 0; i < sd->num_lights; ++i)
        {
            const rt_light& l = sd->lights[i];
            float ft; uint32_t ty = l.type; memcpy(&ft, &ty, 4);
            lights[(size_t)i * 3 + 0] = make_float4(l.origin.x, l.origin.y, l.origin.z, 0.0f);
            lights[(size_t)i * 3 + 1] = make_float4(l.radiance.x, l.radiance.y, l.radiance.z, 0.0f);
            lights[(size_t)i * 3 + 2] = make_float4(ft, 0.0f, 0.0f, 0.0f);
            // shadow rays towards a directional light all share its direction (light.h:57-61: origin * 20000, normalised again
            // by HitSurface): a zero or tiny component makes 1/dir non-finite (RT_SIGN_SLOW) for every one of them
            if (l.type == RT_LIGHT_TYPE_POINT) continue;
            const double len = std::sqrt((double)l.origin.x * l.origin.x + (double)l.origin.y * l.origin.y + (double)l.origin.z * l.origin.z);
            const double lim = len * 0x1p-95;
            if (!(std::fabs((double)l.origin.x) > lim && std::fabs((double)l.origin.y) > lim && std::fabs((double)l.origin.z) > lim)) ++slow_lights;
        }
        s.slow_shadow = slow_lights != 0 && 4u * slow_lights >= sd->num_lights;
    }

    // the indices the shading kernels follow without a check of their own: texture slots, emissive triangles, texel ranges
    int check_tables()
    {
        for (uint32_t i = 0; i < sd->num_materials; ++i)
        {
            // every 8-bit texture slot of a packed material: 0xFF = none (constants.h:35), else an index into textures
            const rt_packed_material& m = sd->materials[i];
            const uint32_t idx[6] = {m.diffuse_albedo >> 24, m.specular_albedo >> 24, (m.roughness_metalness >> 8) & 0xFFu,
                m.roughness_metalness >> 24, (m.ior_emission_idx_transparency >> 8) & 0xFFu, m.ior_emission_idx_transparency >> 24};
            if (!sd->material_texture_indices)
                for (uint32_t t : idx)
                    if (t != RT_INVALID_TEXTURE_IDX && t >= sd->num_textures)
                        return fail(ctx, "rt_scene_upload: material references a texture that does not exist");
        }
        if (sd->material_texture_indices)          // the wide indices replace the packed ones (rt_scene_desc)
            for (size_t i = 0; i < (size_t)sd->num_materials * 6; ++i)
                if (sd->material_texture_indices[i] != 0xFFFFu && sd->material_texture_indices[i] >= sd->num_textures)
                    return fail(ctx, "rt_scene_upload: material_texture_indices references a texture that does not exist");
        for (uint32_t i = 0; i < sd->num_emissive; ++i)
            if (sd->emissive_indices[i] >= nt) return fail(ctx, "rt_scene_upload: emissive index outside the triangle array");
        for (uint32_t i = 0; i < sd->num_textures; ++i)
        {
            const rt_texture& t = sd->textures[i];
            if (t.width <= 0 || t.height <= 0 || t.data_start < 0 ||
                (uint64_t)t.data_start + (uint64_t)t.width * t.height > sd->num_texture_data)
                return fail(ctx, "rt_scene_upload: texture outside texture_data");
        }
        return RT_OK;
    }

    // Re-layout on the device: the reference's arrays go to HBM as they are, three streaming kernels write the child-pair node records and the 64-byte /
    // 128-byte triangle records (relayout_records: they are of the hot path's code object, so rt_hip.hip launches them).  Then, RT_CTX_OPT_DEVICE_FOLD, the
    // reference tree's collapse into 4-wide records from the node array the kernels have just read (device_fold.h), on the same stream, before that array is
    // freed with the stage's other temporaries.
    int relayout_on_device()
    {
        static const char* who = "rt_scene_upload";
        dev::Mem raw_tris, raw_nodes, d_index, d_last, d_err;
        rc |= dev_fill(ctx, who, raw_tris, sd->triangles, (size_t)nt * sizeof(rt_triangle));
        rc |= dev_fill(ctx, who, raw_nodes, sd->nodes, (size_t)nn * sizeof(rt_bvh_node));
        rc |= dev_fill(ctx, who, d_index, interior_index.data(), (size_t)nn * sizeof(uint32_t));
        rc |= dev_fill(ctx, who, d_last, nullptr, (size_t)nt);
        rc |= dev_fill(ctx, who, d_err, nullptr, sizeof(int));
        rc |= scene_array(ctx, &s.nodes, nullptr, (size_t)(n_interior + 1) * 64);   // + the super-root record
        rc |= scene_array(ctx, &s.tris_rt, nullptr, (size_t)nt * 64);
        rc |= scene_array(ctx, &s.tris_sh, nullptr, (size_t)nt * 128);
        if (rc != RT_OK) return RT_ERROR;
        int relayout_err = RL_OK;
        bool ok = hipMemsetAsync(d_last.get(), 0, (size_t)nt, ctx->stream) == hipSuccess &&
                  hipMemsetAsync(d_err.get(), 0, sizeof(int), ctx->stream) == hipSuccess;
        if (ok)
        {
            ok = relayout_records(ctx, raw_nodes.get<const rt_bvh_node>(), nn, raw_tris.get<const rt_triangle>(), nt, sd->num_materials, d_index.get<const uint32_t>(),
                     d_last.get<uint8_t>(), d_err.get<int>(), (float4*)s.nodes, (float4*)s.tris_rt, (float4*)s.tris_sh) == RT_OK &&
                 hipMemcpyAsync((char*)s.nodes + (size_t)n_interior * 64, super_root.data(), 64, hipMemcpyHostToDevice,
                     ctx->stream) == hipSuccess &&
                 hipMemcpyAsync(&relayout_err, d_err.get(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                 hipStreamSynchronize(ctx->stream) == hipSuccess;
        }
        if (ok && relayout_err == RL_OK && ctx->device_fold && ctx->build_wide == 1u && fits_offsets32(nt))
        {
            const bool want_host_copy = ctx->wide_layout != 0u || (may_own && (ctx->shadow_tree == 1u || ctx->closest_tree == 1u));   // the pair layout and the choice by proxy rays work on the host
            folded_on_device = devfold::fold(ctx->stream, raw_nodes.get<const rt_bvh_node>(), nn, sd->nodes[0], nullptr, nullptr, (WideNode**)&s.trees[TREE_REF].recs, &n_wide_dev, &w_entry,
                                             &wide_roots, want_host_copy ? &wide : nullptr, nullptr, &t_dev_fold);
            (void)hipGetLastError();
        }
        if (!ok) return fail(ctx, "rt_scene_upload: device re-layout failed");
        switch (relayout_err)
        {
        case RL_OK: return RT_OK;
        case RL_CHILD_RANGE: return fail(ctx, "rt_scene_upload: child index outside the node array");
        case RL_LEAF_RANGE: return fail(ctx, "rt_scene_upload: leaf range outside the triangle array");
        case RL_AXIS: return fail(ctx, "rt_scene_upload: bad split axis");
        default: return fail(ctx, "rt_scene_upload: material index out of range");
        }
    }

    // the small arrays, as the caller gave them
    void upload_tables()
    {
        rc |= scene_array(ctx, &s.materials, sd->materials, (size_t)sd->num_materials * sizeof(rt_packed_material));
        rc |= scene_array(ctx, &s.textures, sd->textures, (size_t)sd->num_textures * sizeof(rt_texture));
        rc |= scene_array(ctx, &s.texture_data, sd->texture_data, (size_t)sd->num_texture_data * 4);
        rc |= scene_array(ctx, &s.lights, lights.data(), lights.size() * sizeof(float4));
        rc |= scene_array(ctx, &s.env, sd->env_rgba, (size_t)sd->env_width * sd->env_height * 16);
        rc |= scene_array(ctx, &s.emissive, sd->emissive_indices, (size_t)sd->num_emissive * 4);
        if (sd->material_texture_indices)
            rc |= scene_array(ctx, &s.mat_tex16, sd->material_texture_indices, (size_t)sd->num_materials * 6 * sizeof(uint16_t));
        t_device = lap() - t_dev_fold;
    }

    // the 4-wide quantized tree for k_trace_w4, on host threads if the device has not folded it (optional: trees that do not qualify keep the BVH2 kernels)
    // (a SAH collapse can be deeper than the kernel's stack bound allows where two levels at a time are not: try both)
    void fold_reference_tree()
    {
        have_wide = folded_on_device || (ctx->build_wide && fits_offsets32(nt) &&
            ((ctx->build_wide != 2u && build_wide_bvh(sd->nodes, nn, RT_WIDE_SAH, wide, w_entry, &wide_roots)) ||
             build_wide_bvh(sd->nodes, nn, RT_WIDE_TWO_LEVELS, wide, w_entry, &wide_roots)));
        n_wide_ref = folded_on_device ? n_wide_dev : (uint32_t)wide.size();
        WideTree& ref = s.trees[TREE_REF];
        if (have_wide && ctx->wide_layout && !wide.empty())
        {
            pair_layout_by_area(wide, wide_roots, sd->nodes, nn, (const ownbvh::Metric*)nullptr);
            if (folded_on_device && hipMemcpyAsync(ref.recs, wide.data(), wide.size() * sizeof(WideNode), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc |= fail(ctx, "rt_scene_upload: uploading the paired records failed");
        }
        if (!folded_on_device && have_wide) rc |= scene_array(ctx, &ref.recs, wide.data(), wide.size() * sizeof(WideNode));
        ref.n = have_wide ? n_wide_ref : 0u;
        ref.entry = w_entry;
        t_fold = lap() + t_dev_fold;
    }

    // Trees of the backend's own over the reference's leaves (own_bvh.h): one for the shadow rays (exact: an any-hit verdict
    // does not depend on what sits above the leaves) and -- opt-in, tolerance mode -- one for the closest-hit rays.  Which
    // candidate a population walks is MEASURED with proxy rays (tree_select.h); the reference's own topology is a candidate,
    // so the choice is never worse than sharing on that measure.
    void choose_own_trees()
    {
        OwnTree &own_sh = w.own_sh, &own_cl = w.own_cl, &own_sh_dev = w.own_sh_dev;
        // the shadow rays' candidates: the one built on the device is ready first and is measured first; if it wins, the host's build is abandoned
        sh = &own_sh;
        ChoiceInputs shadow_choice;              // (the proxy rays and the reference fold's cost: measured once for both candidates)
        if (try_device_tree)
        {
            own_sh_dev.join();
            (void)hipSetDevice(ctx->device);
            if (own_sh_dev.ok && have_wide && n_wide_ref != 0u && choose_tree(sd, wide, w_entry, true, ctx->shadow_tree, own_sh_dev, s.tree_report, &shadow_choice))
            {
                sh = &own_sh_dev;
                own_sh.cancel_build.store(true);
            }
        }
        own_sh.join(); own_cl.join();
        t_own_wait = lap();
        (void)hipSetDevice(ctx->device);
        auto adopt_own = [&](OwnTree& own, TreeSlot slot)
        {
            WideTree& t = s.trees[slot];
            t.n = (uint32_t)own.wide.size(); t.entry = own.entry;
            if (own.d_wide) t.recs = own.d_wide.release();                                     // folded on the device: the records are there
            else rc |= scene_array(ctx, &t.recs, own.wide.data(), own.wide.size() * sizeof(WideNode));
        };
        if (have_wide && n_wide_ref != 0u && may_own && ctx->shadow_tree)
        {
            have_sh = sh == &own_sh_dev || choose_tree(sd, wide, w_entry, true, ctx->shadow_tree, own_sh, s.tree_report, &shadow_choice);
            if (have_sh) adopt_own(*sh, TREE_SHADOW);
        }
        if (have_wide && n_wide_ref != 0u && may_own && ctx->closest_tree)
        {
            have_cl = choose_tree(sd, wide, w_entry, false, ctx->closest_tree, own_cl, s.tree_report);
            if (have_cl) adopt_own(own_cl, TREE_CLOSEST);
        }
        t_choose = lap();
    }

    // RT_CTX_OPT_ADAPTIVE_FOLD: what the first rt_integrate needs to fold these trees again for its own rays (FoldAdapt)
    void arm_adaptation()
    {
        if (!(adaptation_wanted(ctx, nn) && have_wide && n_wide_ref != 0u && !have_cl)) return;
        FoldAdapt* a = new FoldAdapt();
        a->mode = ctx->adaptive_fold;
        a->device = ctx->device;
        a->device_fold = ctx->device_fold != 0u && ctx->build_wide == 1u;
        a->pairs = ctx->wide_layout != 0u;
        a->min_interval_ms = ctx->adapt_min_interval_ms;
        memset(&a->camera, 0, sizeof(a->camera));
        const rt_bvh_node& root = sd->nodes[0];
        const double ex = (double)root.bounds_max.x - root.bounds_min.x, ey = (double)root.bounds_max.y - root.bounds_min.y, ez = (double)root.bounds_max.z - root.bounds_min.z;
        a->scene_diagonal = std::sqrt(ex * ex + ey * ey + ez * ez);
        w.join_copies();
        if (w.bvh2.size() == nn) a->bvh2.swap(w.bvh2); else a->bvh2.assign(sd->nodes, sd->nodes + nn);
        a->roots = std::move(wide_roots);
        if (have_sh) { a->bvh2_sh = std::move(sh->bvh2); a->roots_sh = std::move(sh->roots); }
        if (a->mode.load() & 16u)
        {
            if (w.tri9.size() == (size_t)nt * 9) a->tri9.swap(w.tri9); else copy_corners(sd->triangles, nt, a->tri9);
        }
        s.adapt = a;
    }

    // the kernels' view of the scene, the flags, the report's `upload:` line; the scene is the context's from here
    void publish()
    {
        s.d.nodes = (const float4*)s.nodes; s.d.tris_rt = (const float4*)s.tris_rt; s.d.tris_sh = (const float4*)s.tris_sh;
        s.d.materials = (const rt_packed_material*)s.materials; s.d.mat_tex16 = (const uint16_t*)s.mat_tex16;
        s.d.textures = (const rt_texture*)s.textures; s.d.texture_data = (const uint32_t*)s.texture_data;
        s.d.lights = (const float4*)s.lights; s.d.light_count = sd->num_lights;
        s.d.env = (const float4*)s.env; s.d.env_w = (int)sd->env_width; s.d.env_h = (int)sd->env_height;
        s.d.gamma_lut = ctx->gamma_lut;
        s.d.emissive = (const uint32_t*)s.emissive; s.d.emissive_count = sd->num_emissive;
        s.d.emissive_nee = (sd->flags & RT_SCENE_EMISSIVE_NEE) && sd->num_emissive ? 1u : 0u;
        s.walk_trees(have_cl ? TREE_CLOSEST : TREE_REF, have_sh ? TREE_SHADOW : TREE_REF);
        s.n_tris = nt;
        s.leaf_starts = new LeafStarts(leaf_starts(sd->nodes, nn, nt));     // what imported records are checked against (rt_scene_import_folds)
        s.wide_ok = have_wide;
        s.offsets32 = fits_offsets32(n_interior + 1) && fits_offsets32(nt);
        if (!s.offsets32)
            fprintf(stderr, "rt_scene_upload: warning: the node or trace-triangle records reach 4 GiB (%u interior nodes, %u triangles): k_trace_w4 and k_trace2 "
                            "address them with 32-bit byte offsets, so every launch takes the per-ray kernel k_trace_v1 -- correct, and several times slower\n",
                n_interior, nt);
        s.valid = true;
        // where the upload's time went (rt_scene_tree_report; bench.py prints it as `setup`)
        char line[400];
        const double t_rest = lap();
        snprintf(line, sizeof(line), "upload: %.3f s = record order on the host %.3f + copies and re-layout kernels %.3f + fold of the reference's tree %.3f (%s) + waiting for the own tree(s) %.3f "
            "(shadow tree: built %s in %.3f, folded in %.3f) + choosing by proxy rays and uploading %.3f + adaptation state %.3f (%u triangles, %u nodes, %u + %u wide records)\n",
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t_upload).count(), t_layout, t_device, t_fold, folded_on_device ? "on the device" : "on host threads", t_own_wait,
            sh->built_on_device ? "on the device (PLOC)" : (try_device_tree ? "on host threads (the device-built candidate did not win its measurement)" : "on host threads"),
            sh->build_seconds, sh->fold_seconds, t_choose, t_rest, nt, nn, s.trees[TREE_REF].n, s.trees[TREE_SHADOW].n);
        s.tree_report += line;
        ctx->scene = s;
        s = Scene();
    }
};
} // namespace

extern "C" {

static void refit_arm(rt_ctx* ctx, const rt_scene_desc* sd, uint32_t n_pairs);   // RT_CTX_OPT_REFITTABLE (below, with the refit)

// ---- scene -----------------------------------------------------------------
int rt_scene_upload(rt_ctx* ctx, const rt_scene_desc* sd)
{
    if (!ctx || !sd) return fail(ctx, "rt_scene_upload: NULL argument");
    if (!sd->triangles || sd->num_triangles == 0) return fail(ctx, "rt_scene_upload: no triangles");
    if (!sd->nodes || sd->num_nodes == 0) return fail(ctx, "rt_scene_upload: no BVH nodes");
    if (!sd->materials || sd->num_materials == 0) return fail(ctx, "rt_scene_upload: no materials");
    if (!sd->env_rgba || sd->env_width == 0 || sd->env_height == 0)
        return fail(ctx, "rt_scene_upload: no environment image");
    (void)hipSetDevice(ctx->device);
    if (quiesce(ctx) != RT_OK) return RT_ERROR;      // nothing may still read the scene that is about to be freed
    free_scene(ctx->scene);
    ++ctx->scene_uploads;
    ++ctx->upload_epoch;
    ctx->refit_index = 0;
    Upload u(ctx, sd);                               // any return before publish(): the context has no scene, the host builds are given up
    u.start_workers();
    if (u.order_records() != RT_OK) return RT_ERROR;
    u.stage_lights();
    if (u.check_tables() != RT_OK) return RT_ERROR;
    if (u.relayout_on_device() != RT_OK) return RT_ERROR;
    u.upload_tables();
    u.fold_reference_tree();
    u.choose_own_trees();
    if (u.rc != RT_OK) return RT_ERROR;
    u.arm_adaptation();
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // host staging vectors die here
    u.publish();
    if (ctx->refittable) refit_arm(ctx, sd, u.n_interior + 1u);
    return RT_OK;
}

// ---- the refit: rt_scene_refit / rt_scene_refit_buffer / rt_debug_refit, the bookkeeping around refit.hip's kernels ------------
// After a successful refit the context behaves as a fresh one would after rt_scene_upload of the moved triangles with the node array "same topology, same
// split axes, bounds refitted".

// RT_CTX_OPT_REFITTABLE at the end of rt_scene_upload: the links of the child-pair records and of the 4-wide trees the scene starts with
static bool refit_link_trees(rt_ctx* ctx);
static void refit_arm(rt_ctx* ctx, const rt_scene_desc* sd, uint32_t n_pairs)
{
    Scene& s = ctx->scene;
    s.refit_wide_built = s.wide_ok;
    s.n_materials = sd->num_materials;
    if (!refit::leaves_partition(sd->nodes, sd->num_nodes, sd->num_triangles)) { s.refit_refusal = "the leaves of the uploaded node array are not consecutive ranges that cover the triangle array"; return; }
    s.refit = new refit::State();
    if (!refit::prepare(ctx->stream, *s.refit, (const float4*)s.nodes, n_pairs) || !refit_link_trees(ctx) || hipStreamSynchronize(ctx->stream) != hipSuccess)
    {
        (void)hipGetLastError();
        refit::release(*s.refit); delete s.refit; s.refit = nullptr;
        s.refit_refusal = "the refit state could not be allocated at upload";
    }
    if (!s.refit || !ctx->refit_motion) return;
    // RT_CTX_OPT_REFIT_MOTION: room for the pose a refit replaces; without it the option is off for this scene
    char line[200];
    if (hipMalloc(&s.pose_snap, (size_t)s.n_tris * 96u) != hipSuccess)
    {
        (void)hipGetLastError();
        s.pose_snap = nullptr;
        snprintf(line, sizeof(line), "previous pose: could not be allocated at upload, RT_CTX_OPT_REFIT_MOTION is treated as off\n");
    }
    else snprintf(line, sizeof(line), "previous pose: RT_CTX_OPT_REFIT_MOTION keeps 96 bytes per triangle (%.1f MB)\n", (double)s.n_tris * 96.0 / 1e6);
    s.tree_report += line;
}

// the 4-wide trees the scene holds NOW (an adaptation or rt_scene_import_folds may have replaced the records since the links were made)
static bool refit_link_trees(rt_ctx* ctx)
{
    Scene& s = ctx->scene;
    const WideTree &ref = s.trees[TREE_REF], &sh = s.trees[TREE_SHADOW];
    const bool wide = s.refit_wide_built && ref.recs && ref.n != 0u;
    const bool own_sh = wide && s.shadow == TREE_SHADOW && sh.recs && sh.n != 0u;           // tree 1: only records of the shadow rays' own
    return refit::link_tree(ctx->stream, *s.refit, 0, wide ? (WideNode*)ref.recs : nullptr, ref.n, s.d.w_entry_ref) &&
           refit::link_tree(ctx->stream, *s.refit, 1, own_sh ? (WideNode*)sh.recs : nullptr, sh.n, s.d.w_sh_entry_ref);
}

} // extern "C": the next two are context.h's, for the producers of moved triangles too (scene_moved.cpp)

int context::refit_device(rt_ctx* ctx, const rt_triangle* d_tris, const char* who)
{
    Scene& s = ctx->scene;
    const std::string name(who);
    // read-only first: a refused refit leaves the scene untouched
    switch (refit::validate(ctx->stream, *s.refit, d_tris, s.n_tris, s.n_materials))
    {
    case refit::OK: break;
    case refit::BAD_POSITION: return fail(ctx, name + ": a triangle has a non-finite position");
    case refit::BAD_MATERIAL: return fail(ctx, name + ": material index out of range");
    default: (void)hipGetLastError(); return fail(ctx, name + ": the validation kernel failed");
    }
    if (quiesce(ctx) != RT_OK) return RT_ERROR;                            // nothing may still read what is about to be rewritten
    // an adaptation's host copies (the binary trees, the triangles' corners) are stale from here on: it is retired -- one in flight is cancelled and waited
    // for -- and the records adapted so far stay in use
    const bool had_adapt = s.adapt != nullptr;
    if (s.adapt) { drop_fold_adapt(s.adapt); s.adapt = nullptr; (void)hipSetDevice(ctx->device); }
    // RT_CTX_OPT_REFIT_MOTION: the pose about to be replaced, while the shading records still hold it
    if (s.pose_snap)
    {
        s.pose_valid = false;
        HIPCHK(ctx, filt::snapshot_pose(ctx->stream, (const float4*)s.tris_sh, s.n_tris, (float4*)s.pose_snap));
    }
    const auto t0 = std::chrono::steady_clock::now();
    refit::Result res;
    if (!refit_link_trees(ctx) ||
        !refit::run(ctx->stream, *s.refit, d_tris, s.n_tris, (float4*)s.tris_rt, (float4*)s.tris_sh, (float4*)s.nodes, s.d.entry_ref, res) || res.error != refit::OK)
    {
        (void)hipGetLastError();
        s.valid = false;                                                   // half-written records: upload again
        return fail(ctx, name + ": the refit kernels failed; the scene is no longer valid, upload it again");
    }
    for (int k = 0; k < 3; ++k) { s.d.root_min[k] = res.root_min[k]; s.d.root_max[k] = res.root_max[k]; }
    // a record that no longer qualifies for k_trace_w4: the BVH2 kernels, as upload does for such trees; a later refit that qualifies switches back
    const bool fallback = s.refit_wide_built && (res.wide_bad[0] || res.wide_bad[1]);
    s.wide_ok = s.refit_wide_built && !fallback;
    ++ctx->scene_uploads;                                                  // guide caches, temporal histories, measured choices: dropped as on upload
    ++s.refits;
    ++ctx->refit_index;
    s.pose_valid = s.pose_snap != nullptr;
    {
        char pose[96] = "";
        if (s.pose_snap) snprintf(pose, sizeof(pose), " + %.1f MB for the previous pose, 96 bytes per triangle", (double)s.n_tris * 96.0 / 1e6);
        char line[500];
        snprintf(line, sizeof(line), "refit %llu: %.3f ms on the device (%u triangles, %u child-pair records, %u + %u wide records, %.1f MB kept for it%s); %s; %s\n",
            (unsigned long long)s.refits, 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), s.n_tris, s.refit->n_pairs,
            s.refit->trees[0].n, s.refit->trees[1].n, (double)s.refit->bytes / 1e6, pose,
            fallback ? "a 4-wide record no longer qualifies -> the BVH2 kernels until a refit qualifies again" : (s.refit_wide_built ? "the 4-wide trees qualify" : "no 4-wide tree"),
            had_adapt || s.adapt_retired ? "the fold adaptation is retired (the records adapted so far stay)" : "no fold adaptation");
        s.adapt_retired = s.adapt_retired || had_adapt;
        replace_report_line(s.tree_report, "refit ", line);
    }
    return RT_OK;
}

int context::refit_refused(rt_ctx* ctx, const char* who, uint64_t count_or_bytes, bool bytes)
{
    const std::string name(who);
    Scene& s = ctx->scene;
    if (!ctx->scene.valid) return fail(ctx, name + ": no scene");
    if (!s.refit) return fail(ctx, name + (s.refit_refusal.empty() ? ": RT_CTX_OPT_REFITTABLE was off when the scene was uploaded" : ": " + s.refit_refusal));
    if (ctx->closest_tree != 0u || s.trees[TREE_CLOSEST].recs) return fail(ctx, name + ": not in the tolerance mode (RT_CTX_OPT_CLOSEST_TREE != 0)");
    if (bytes ? count_or_bytes != (uint64_t)s.n_tris * sizeof(rt_triangle) : count_or_bytes != s.n_tris)
        return fail(ctx, name + ": the triangle count differs from the uploaded scene's");
    return RT_OK;
}

extern "C" {

int rt_scene_refit_buffer(rt_ctx* ctx, rt_buffer* triangles)
{
    if (!ctx || !triangles) return fail(ctx, "rt_scene_refit_buffer: NULL argument");
    if (triangles->ctx != ctx) return fail(ctx, "rt_scene_refit_buffer: the buffer belongs to another context");
    if (refit_refused(ctx, "rt_scene_refit_buffer", triangles->bytes, true) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    return refit_device(ctx, (const rt_triangle*)triangles->ptr, "rt_scene_refit_buffer");
}

int rt_scene_refit(rt_ctx* ctx, const rt_triangle* triangles, uint32_t num_triangles)
{
    if (!ctx || !triangles) return fail(ctx, "rt_scene_refit: NULL argument");
    if (refit_refused(ctx, "rt_scene_refit", num_triangles, false) != RT_OK) return RT_ERROR;
    (void)hipSetDevice(ctx->device);
    dev::Mem d_tris;
    if (dev_fill(ctx, "rt_scene_refit", d_tris, triangles, (size_t)num_triangles * sizeof(rt_triangle)) != RT_OK) return RT_ERROR;
    const int rc = refit_device(ctx, d_tris.get<const rt_triangle>(), "rt_scene_refit");
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int rt_debug_refit(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, const rt_triangle* triangles, uint32_t num_triangles, const void* records, uint32_t num_records,
    uint32_t entry_ref, rt_bvh_node* out_nodes, void* out_records)
{
    std::string error;
    bool bad = false;
    if (ctx) (void)hipSetDevice(ctx->device);
    const bool ok = ctx ? refit::debug_device(ctx->stream, nodes, num_nodes, triangles, num_triangles, (const WideNode*)records, num_records, entry_ref, out_nodes, (WideNode*)out_records, &bad, error)
                        : refit::debug_host(nodes, num_nodes, triangles, num_triangles, (const WideNode*)records, num_records, entry_ref, out_nodes, (WideNode*)out_records, &bad, error);
    if (!ok) return fail(ctx, "rt_debug_refit: " + error);
    return bad ? RT_REFIT_DISQUALIFIED : RT_OK;
}

// ---- one adaptation per process GROUP (round 6) ----------------------------------------------------------------------------------------
// N ranks that tile one image hold the same scene and probe the same low-resolution frame: N identical adaptations (tree rotations on host threads: seconds)
// for identical records.  Instead one rank adapts and the others TAKE its 4-wide records: rt_scene_export_folds copies the context's current records (the
// closest-hit rays' and the shadow rays', as adapted so far) to the host, the launcher's own channel carries them (torch.distributed, MPI, a file: 64 bytes
// per record, ~240 MB for the 2.8 M-triangle scene), rt_scene_import_folds puts them in place of the receiver's own and switches its adaptation off.  The
// records are indices into the triangle records every rank made from the same scene, so nothing else travels.  Exactness is the fold's: any fold of the same
// binary tree over the same leaves gives the same results -- and the importer checks that the records ARE such a fold as far as the
// walks depend on it (rtw::check_fold): a tree from the entry, no deeper than the walks' stacks, every leaf of this scene reached exactly once by its first
// triangle, slot counts and frames within what the kernels' arithmetic takes.  What it cannot check is what only the binary tree could tell: the boxes.
int rt_scene_export_folds(rt_ctx* ctx, void* closest_records, void* shadow_records, uint32_t capacity, uint32_t* n_closest, uint32_t* n_shadow, uint32_t* entries2)
{
    if (!ctx || !n_closest || !n_shadow) return fail(ctx, "rt_scene_export_folds: NULL argument");
    Scene& s = ctx->scene;
    if (!s.valid || !s.wide_ok || !s.trees[TREE_REF].recs) return fail(ctx, "rt_scene_export_folds: the scene has no 4-wide tree");
    (void)hipSetDevice(ctx->device);
    const bool own_shadow = s.shadow == TREE_SHADOW;
    const uint32_t n_cl = s.closest_tree().n;                                                 // (tolerance mode: the closest-hit rays' own tree)
    *n_closest = n_cl;
    *n_shadow = own_shadow ? s.shadow_tree().n : 0u;
    if (entries2) { entries2[0] = s.d.w_entry_ref; entries2[1] = s.d.w_sh_entry_ref; }
    if (!closest_records) return RT_OK;                                                       // size query
    if (n_cl > capacity || *n_shadow > capacity) return fail(ctx, "rt_scene_export_folds: capacity too small");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(closest_records, s.d.wnodes, (size_t)n_cl * sizeof(WideNode), hipMemcpyDeviceToHost));
    if (own_shadow && shadow_records) HIPCHK(ctx, hipMemcpy(shadow_records, s.d.wnodes_sh, (size_t)s.shadow_tree().n * sizeof(WideNode), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_import_folds(rt_ctx* ctx, const void* closest_records, uint32_t n_closest, uint32_t entry_closest, const void* shadow_records, uint32_t n_shadow, uint32_t entry_shadow)
{
    if (!ctx || (!closest_records && n_closest != 0)) return fail(ctx, "rt_scene_import_folds: NULL argument");
    // a scene whose root is a leaf has no 4-wide tree: rt_scene_export_folds refuses it ("the scene has no 4-wide tree"), so there is nothing to take
    if (n_closest == 0) return fail(ctx, "rt_scene_import_folds: no records (a scene whose root is a leaf has no 4-wide tree; rt_scene_export_folds gives none for it)");
    Scene& s = ctx->scene;
    if (!s.valid || !s.wide_ok) return fail(ctx, "rt_scene_import_folds: the scene has no 4-wide tree to replace (upload it first, with RT_CTX_OPT_WIDE_BVH = 1)");
    if (n_closest >= (1u << 26) || n_shadow >= (1u << 26)) return fail(ctx, "rt_scene_import_folds: too many records");
    (void)hipSetDevice(ctx->device);
    // what records from outside must be before a walk may see them: a tree over this scene's leaves, no deeper than the walks' stacks, frames within the
    // walks' arithmetic (check_fold, wide_bvh.cpp; DESIGN.md, "one adaptation per group").  Both arrays against the same leaves: the shadow rays' own tree is
    // built over the reference's.  A refusal leaves the context as it was.
    if (!s.leaf_starts) return fail(ctx, "rt_scene_import_folds: the scene has no record of its leaves");
    const FoldDefect bad_cl = check_fold((const WideNode*)closest_records, n_closest, entry_closest, *s.leaf_starts);
    if (bad_cl != FoldDefect::NONE) return fail(ctx, std::string("rt_scene_import_folds: the closest-hit records do not fit this scene (") + fold_defect_text(bad_cl) + ")");
    if (n_shadow && !shadow_records) return fail(ctx, "rt_scene_import_folds: the shadow records do not fit this scene (a count without records)");
    const FoldDefect bad_sh = n_shadow ? check_fold((const WideNode*)shadow_records, n_shadow, entry_shadow, *s.leaf_starts) : FoldDefect::NONE;
    if (bad_sh != FoldDefect::NONE) return fail(ctx, std::string("rt_scene_import_folds: the shadow records do not fit this scene (") + fold_defect_text(bad_sh) + ")");
    // nothing in flight may still read the records that go: batches traced ahead are dropped, every stream drains, an adaptation of this context's own is abandoned
    if (quiesce(ctx) != RT_OK) return RT_ERROR;
    if (s.adapt) { drop_fold_adapt(s.adapt); s.adapt = nullptr; }
    dev::Mem cl, sh;
    int rc = dev_fill(ctx, "rt_scene_import_folds", cl, closest_records, (size_t)n_closest * sizeof(WideNode));
    if (rc == RT_OK && n_shadow) rc = dev_fill(ctx, "rt_scene_import_folds", sh, shadow_records, (size_t)n_shadow * sizeof(WideNode));
    if (rc == RT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, "rt_scene_import_folds: upload failed");
    if (rc != RT_OK) { (void)hipGetLastError(); return RT_ERROR; }
    // the tree the closest-hit rays walk (their own in the tolerance mode) and the shadow rays' own are replaced; without shadow records the shadow rays
    // walk what the closest-hit rays walk
    dev::Mem old_cl(s.replace_tree(s.closest, WideTree{cl.release(), n_closest, entry_closest}).recs);
    dev::Mem old_sh(s.replace_tree(TREE_SHADOW, WideTree{sh.release(), n_shadow, entry_shadow}).recs);
    s.walk_trees(s.closest, n_shadow ? TREE_SHADOW : s.closest);
    char line[200];
    snprintf(line, sizeof(line), "imported folds: %u closest-hit + %u shadow records taken from another context of the group; this context's own adaptation is off\n", n_closest, n_shadow);
    replace_report_line(s.tree_report, "imported folds", line);
    return RT_OK;
}

// ---- the tree report, and the rt_debug_* entry points that expose the backend's tree work on its own (folds, own trees, tree choice, adaptation halves,
// pair layout, the device fold) to the tests and tools -------------------------------------------------------------------------------------------------

int rt_debug_wide_bvh(const rt_bvh_node* nodes, uint32_t num_nodes, int collapse, void* records, uint32_t* roots, uint32_t capacity,
    uint32_t* num_records, uint32_t* entry_ref)
{
    if (!nodes || num_nodes == 0 || !num_records || !entry_ref) return fail(nullptr, "rt_debug_wide_bvh: NULL argument");
    std::vector<WideNode> wide;
    uint32_t entry = 0;
    std::vector<uint32_t> folded;
    if (!build_wide_bvh(nodes, num_nodes, collapse == 2 ? RT_WIDE_TWO_LEVELS : RT_WIDE_SAH, wide, entry, &folded))
        return fail(nullptr, "rt_debug_wide_bvh: the tree does not qualify for the 4-wide layout (bounds not finite / not nested, or too deep)");
    *num_records = (uint32_t)wide.size();
    *entry_ref = entry;
    if (records)
    {
        if (wide.size() > capacity) return fail(nullptr, "rt_debug_wide_bvh: capacity too small");
        memcpy(records, wide.data(), wide.size() * sizeof(WideNode));
        if (roots) memcpy(roots, folded.data(), folded.size() * sizeof(uint32_t));
    }
    return RT_OK;
}

const char* rt_scene_tree_report(rt_ctx* ctx)
{
    if (!ctx) return "";
    if ((ctx->query.bytes() == 0u && ctx->bake.bytes() == 0u) || !ctx->scene.valid) return ctx->scene.tree_report.c_str();
    // what the context keeps for its ray queries and bakes (query_host.h, bake_host.h) is the context's, not the scene's: its line is added here, when the
    // report is asked for
    char line[300];
    if (ctx->bake.bytes() == 0u)
        snprintf(line, sizeof(line), "ray queries: %.1f MB kept on the device (stack spill area %.1f MB + staging)\n", (double)ctx->query.bytes() / 1e6,
            (double)ctx->query.spill_bytes() / 1e6);
    else
        snprintf(line, sizeof(line), "ray queries: %.1f MB kept on the device (stack spill area %.1f MB + staging; of that the bakes' %.1f MB: spill area %.1f MB + staging)\n",
            (double)(ctx->query.bytes() + ctx->bake.bytes()) / 1e6, (double)(ctx->query.spill_bytes() + ctx->bake.spill_bytes()) / 1e6, (double)ctx->bake.bytes() / 1e6,
            (double)ctx->bake.spill_bytes() / 1e6);
    ctx->report_out = ctx->scene.tree_report + line;
    return ctx->report_out.c_str();
}

int rt_debug_device_fold(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, double iso_weight, const float* dirs, uint32_t n_dirs, const double* weights,
    void* records, uint32_t* roots, uint32_t capacity, uint32_t* num_records, uint32_t* entry_ref, double* seconds)
{
    if (!ctx || !nodes || num_nodes == 0 || !num_records || !entry_ref) return fail(ctx, "rt_debug_device_fold: NULL argument");
    (void)hipSetDevice(ctx->device);
    ownbvh::Metric m;
    const bool with_metric = iso_weight >= 0.0;
    if (with_metric)
    {
        m.iso = iso_weight;
        for (uint32_t i = 0; i < n_dirs && dirs; ++i) m.dirs.push_back({std::fabs((double)dirs[3 * i]), std::fabs((double)dirs[3 * i + 1]), std::fabs((double)dirs[3 * i + 2])});
    }
    dev::Mem d_nodes;
    if (dev_fill(ctx, "rt_debug_device_fold", d_nodes, nodes, (size_t)num_nodes * sizeof(rt_bvh_node)) != RT_OK) return RT_ERROR;
    WideNode* d_recs = nullptr;
    std::vector<uint32_t> folded;
    std::vector<WideNode> wide;
    const bool ok = devfold::fold(ctx->stream, d_nodes.get<const rt_bvh_node>(), num_nodes, nodes[0], with_metric ? &m : nullptr, weights, &d_recs, num_records, entry_ref, &folded, &wide, nullptr, seconds);
    const dev::Mem folded_records(d_recs);                          // the fold's records are the caller's to free; only the host copies are wanted here
    (void)hipStreamSynchronize(ctx->stream);
    if (!ok) return fail(ctx, "rt_debug_device_fold: the tree does not qualify for the 4-wide layout, or the device path failed");
    if (records)
    {
        if (wide.size() > capacity) return fail(ctx, "rt_debug_device_fold: capacity too small");
        memcpy(records, wide.data(), wide.size() * sizeof(WideNode));
        if (roots) memcpy(roots, folded.data(), folded.size() * sizeof(uint32_t));
    }
    return RT_OK;
}

int rt_debug_device_tree(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, double iso_weight, const float* dirs, uint32_t n_dirs, rt_bvh_node* out_nodes, uint32_t capacity,
    uint32_t* num_out, double* seconds, uint32_t* rounds, uint32_t radius, const float* frame_dir, double stretch)
{
    if (!ctx || !nodes || num_nodes == 0 || !num_out) return fail(ctx, "rt_debug_device_tree: NULL argument");
    (void)hipSetDevice(ctx->device);
    ownbvh::Metric m;
    m.iso = iso_weight;
    for (uint32_t i = 0; i < n_dirs && dirs; ++i) m.dirs.push_back({std::fabs((double)dirs[3 * i]), std::fabs((double)dirs[3 * i + 1]), std::fabs((double)dirs[3 * i + 2])});
    dev::Mem d_nodes;
    if (dev_fill(ctx, "rt_debug_device_tree", d_nodes, nodes, (size_t)num_nodes * sizeof(rt_bvh_node)) != RT_OK) return RT_ERROR;
    rt_bvh_node* d_tree = nullptr;
    uint32_t n = 0;
    std::vector<rt_bvh_node> tree;
    const bool ok = devfold::build_tree(ctx->stream, d_nodes.get<const rt_bvh_node>(), num_nodes, nodes[0], &m, &d_tree, &n, &tree, nullptr, seconds, rounds, frame_dir, radius, stretch);
    const dev::Mem built_tree(d_tree);                              // likewise: only the host copy is wanted here
    (void)hipStreamSynchronize(ctx->stream);
    if (!ok) return fail(ctx, "rt_debug_device_tree: nothing to build (leaf root), or the device path failed");
    *num_out = n;
    if (out_nodes)
    {
        if (n > capacity) return fail(ctx, "rt_debug_device_tree: capacity too small");
        memcpy(out_nodes, tree.data(), tree.size() * sizeof(rt_bvh_node));
    }
    return RT_OK;
}

int rt_debug_pair_layout(const rt_bvh_node* nodes, uint32_t num_nodes, void* records, uint32_t* roots, uint32_t num_records)
{
    if (!nodes || !records || !roots || num_nodes == 0) return fail(nullptr, "rt_debug_pair_layout: NULL argument");
    std::vector<WideNode> wide((const WideNode*)records, (const WideNode*)records + num_records);
    std::vector<uint32_t> r(roots, roots + num_records);
    pair_layout_by_area(wide, r, nodes, num_nodes, (const ownbvh::Metric*)nullptr);
    memcpy(records, wide.data(), wide.size() * sizeof(WideNode));
    memcpy(roots, r.data(), r.size() * sizeof(uint32_t));
    return RT_OK;
}

// rt_scene_import_folds' check without a context (no HIP call): are `records` a fold the walks can take over the leaves of `nodes`?
int rt_debug_check_folds(const rt_bvh_node* nodes, uint32_t num_nodes, const void* records, uint32_t num_records, uint32_t entry_ref)
{
    if (!nodes || num_nodes == 0 || (!records && num_records != 0)) return fail(nullptr, "rt_debug_check_folds: NULL argument");
    if (num_records >= (1u << 26)) return fail(nullptr, "rt_debug_check_folds: too many records");
    uint64_t n_tris = 0;                                                // the triangle array ends where the last leaf does
    for (uint32_t i = 0; i < num_nodes; ++i)
        if ((nodes[i].num_primitives_axis >> 16) != 0u) n_tris = std::max<uint64_t>(n_tris, (uint64_t)nodes[i].offset + (nodes[i].num_primitives_axis >> 16));
    if (n_tris >= RT_LEAF_BIT) return fail(nullptr, "rt_debug_check_folds: a leaf's triangles lie beyond what a ref can hold");
    const FoldDefect bad = check_fold((const WideNode*)records, num_records, entry_ref, leaf_starts(nodes, num_nodes, (uint32_t)n_tris));
    if (bad != FoldDefect::NONE) return fail(nullptr, std::string("rt_debug_check_folds: the records do not fit this scene (") + fold_defect_text(bad) + ")");
    return RT_OK;
}

int rt_debug_wide_bvh_weights(const rt_bvh_node* nodes, uint32_t num_nodes, const double* weights, void* records, uint32_t* roots, uint32_t capacity,
    uint32_t* num_records, uint32_t* entry_ref)
{
    if (!nodes || num_nodes == 0 || !weights || !num_records || !entry_ref) return fail(nullptr, "rt_debug_wide_bvh_weights: NULL argument");
    std::vector<WideNode> wide;
    std::vector<uint32_t> folded;
    uint32_t entry = 0;
    if (!build_wide_bvh(nodes, num_nodes, RT_WIDE_SAH, wide, entry, &folded, nullptr, weights)) return fail(nullptr, "rt_debug_wide_bvh_weights: the tree does not qualify for the 4-wide layout");
    *num_records = (uint32_t)wide.size();
    *entry_ref = entry;
    if (records)
    {
        if (wide.size() > capacity) return fail(nullptr, "rt_debug_wide_bvh_weights: capacity too small");
        memcpy(records, wide.data(), wide.size() * sizeof(WideNode));
        if (roots) memcpy(roots, folded.data(), folded.size() * sizeof(uint32_t));
    }
    return RT_OK;
}

int rt_debug_choose_tree(const rt_scene_desc* sd, int shadow, uint32_t mode, void* records, uint32_t capacity, uint32_t* num_records,
    uint32_t* entry_ref, char* report, size_t report_len)
{
    if (!sd || !sd->nodes || !sd->triangles || !num_records || !entry_ref) return fail(nullptr, "rt_debug_choose_tree: NULL argument");
    std::vector<WideNode> ref_wide;
    uint32_t ref_entry = 0;
    if (!build_wide_bvh(sd->nodes, sd->num_nodes, RT_WIDE_SAH, ref_wide, ref_entry) || ref_wide.empty())
        return fail(nullptr, "rt_debug_choose_tree: the tree does not qualify for the 4-wide layout");
    std::string rep;
    OwnTree own;
    own.start(sd, shadow != 0, mode);
    const bool picked = choose_tree(sd, ref_wide, ref_entry, shadow != 0, mode, own, rep);
    const std::vector<WideNode>& w = picked ? own.wide : ref_wide;
    *num_records = (uint32_t)w.size();
    *entry_ref = picked ? own.entry : ref_entry;
    if (report && report_len) snprintf(report, report_len, "%s", rep.c_str());
    if (records)
    {
        if (w.size() > capacity) return fail(nullptr, "rt_debug_choose_tree: capacity too small");
        memcpy(records, w.data(), w.size() * sizeof(WideNode));
    }
    return RT_OK;
}

int rt_debug_own_bvh(const rt_bvh_node* nodes, uint32_t num_nodes, double iso_weight, const float* dirs, uint32_t n_dirs,
    rt_bvh_node* out_nodes, uint32_t capacity, uint32_t* num_out)
{
    if (!nodes || num_nodes == 0 || !num_out) return fail(nullptr, "rt_debug_own_bvh: NULL argument");
    ownbvh::Metric m;
    m.iso = iso_weight;
    for (uint32_t i = 0; i < n_dirs && dirs; ++i) m.dirs.push_back({std::fabs((double)dirs[3 * i]), std::fabs((double)dirs[3 * i + 1]), std::fabs((double)dirs[3 * i + 2])});
    std::vector<rt_bvh_node> own;
    if (!ownbvh::build(nodes, num_nodes, m, own)) return fail(nullptr, "rt_debug_own_bvh: nothing to build (leaf root) or the node array is not a tree");
    *num_out = (uint32_t)own.size();
    if (out_nodes)
    {
        if (own.size() > capacity) return fail(nullptr, "rt_debug_own_bvh: capacity too small");
        memcpy(out_nodes, own.data(), own.size() * sizeof(rt_bvh_node));
    }
    return RT_OK;
}

int rt_debug_wide_bvh_metric(const rt_bvh_node* nodes, uint32_t num_nodes, double iso_weight, const float* dirs, uint32_t n_dirs,
    void* records, uint32_t capacity, uint32_t* num_records, uint32_t* entry_ref)
{
    if (!nodes || num_nodes == 0 || !num_records || !entry_ref) return fail(nullptr, "rt_debug_wide_bvh_metric: NULL argument");
    ownbvh::Metric m;
    m.iso = iso_weight;
    for (uint32_t i = 0; i < n_dirs && dirs; ++i) m.dirs.push_back({std::fabs((double)dirs[3 * i]), std::fabs((double)dirs[3 * i + 1]), std::fabs((double)dirs[3 * i + 2])});
    std::vector<WideNode> wide;
    uint32_t entry = 0;
    if (!build_wide_bvh(nodes, num_nodes, RT_WIDE_SAH, wide, entry, nullptr, &m))
        return fail(nullptr, "rt_debug_wide_bvh_metric: the tree does not qualify for the 4-wide layout");
    *num_records = (uint32_t)wide.size();
    *entry_ref = entry;
    if (records)
    {
        if (wide.size() > capacity) return fail(nullptr, "rt_debug_wide_bvh_metric: capacity too small");
        memcpy(records, wide.data(), wide.size() * sizeof(WideNode));
    }
    return RT_OK;
}

// The adaptation's crossing counts on their own: the host's walk (ctx == NULL) or k_count_box_passes on ctx's device -- the same rule, compared count for count
// by tests/test_gpu_tree_edges.py.
int rt_debug_count_box_passes(rt_ctx* ctx, const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays,
    uint32_t* counts, unsigned long long* truncated)
{
    if (!nodes || num_nodes == 0 || !counts || (n_rays != 0 && (!origins_tmax || !directions))) return fail(ctx, "rt_debug_count_box_passes: NULL argument");
    // what both walks take for granted (FoldAdapt's trees have passed build_wide_bvh): every interior node's children lie inside the array
    for (uint32_t i = 0; i < num_nodes; ++i)
        if ((nodes[i].num_primitives_axis >> 16) == 0u && (i + 1u >= num_nodes || nodes[i].offset >= num_nodes || nodes[i].offset <= i + 1u))
            return fail(ctx, "rt_debug_count_box_passes: the node array is not a tree in the reference's layout");
    std::vector<float4> o(n_rays), d(n_rays);
    for (uint32_t i = 0; i < n_rays; ++i)
    {
        o[i] = make_float4(origins_tmax[4 * i], origins_tmax[4 * i + 1], origins_tmax[4 * i + 2], origins_tmax[4 * i + 3]);
        d[i] = make_float4(directions[4 * i], directions[4 * i + 1], directions[4 * i + 2], 0.0f);
    }
    std::vector<uint32_t> got;
    uint64_t cut_short = 0;
    if (!ctx)
    {
        std::atomic<bool> cancel{false};
        std::atomic<uint64_t> n_cut{0};
        count_box_passes(nodes, num_nodes, o.data(), d.data(), o.size(), got, cancel, &n_cut);
        cut_short = n_cut.load();
    }
    else
    {
        (void)hipSetDevice(ctx->device);
        dev::Mem d_nodes;
        if (dev_fill(ctx, "rt_debug_count_box_passes", d_nodes, nodes, (size_t)num_nodes * sizeof(rt_bvh_node)) != RT_OK) return RT_ERROR;
        const bool ok = devfold::count_box_passes(ctx->stream, d_nodes.get<const rt_bvh_node>(), num_nodes, o.data(), d.data(), o.size(), got, &cut_short);
        (void)hipStreamSynchronize(ctx->stream);
        if (!ok) return fail(ctx, "rt_debug_count_box_passes: the device path failed");
    }
    memcpy(counts, got.data(), (size_t)num_nodes * sizeof(uint32_t));
    if (truncated) *truncated = cut_short;
    return RT_OK;
}

// RT_CTX_OPT_ADAPTIVE_FOLD's host half on its own (no device): the surface-area fold of `nodes`, then the fold adapted to `n_rays` rays
// (origin.xyz + t_max in .w, direction.xyz) -- the records of the latter, and what both cost those rays (box passes at record roots).
int rt_debug_adapt_fold(const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays,
    void* records, uint32_t* roots, uint32_t capacity, uint32_t* num_records, uint32_t* entry_ref, double* cost2, int* cheaper)
{
    if (!nodes || num_nodes == 0 || !origins_tmax || !directions || !num_records || !entry_ref) return fail(nullptr, "rt_debug_adapt_fold: NULL argument");
    std::vector<rt_bvh_node> tree(nodes, nodes + num_nodes);
    std::vector<WideNode> wide, adapted;
    std::vector<uint32_t> wide_roots;
    uint32_t entry = 0;
    if (!build_wide_bvh(nodes, num_nodes, RT_WIDE_SAH, wide, entry, &wide_roots) || wide.empty())
        return fail(nullptr, "rt_debug_adapt_fold: the tree does not qualify for the 4-wide layout");
    std::vector<float4> o(n_rays), d(n_rays);
    for (uint32_t i = 0; i < n_rays; ++i)
    {
        o[i] = make_float4(origins_tmax[4 * i], origins_tmax[4 * i + 1], origins_tmax[4 * i + 2], origins_tmax[4 * i + 3]);
        d[i] = make_float4(directions[4 * i], directions[4 * i + 1], directions[4 * i + 2], 0.0f);
    }
    double cost[2] = {0.0, 0.0};
    std::atomic<bool> cancel{false};
    std::vector<uint32_t> adapted_roots;
    const bool better = refold_for_rays(tree, o, d, wide_roots, adapted, entry, cost, cancel, &adapted_roots);
    if (adapted.empty()) return fail(nullptr, "rt_debug_adapt_fold: no adapted fold (no ray passed the root box, or the weighted fold is too deep)");
    if (cost2) { cost2[0] = cost[0]; cost2[1] = cost[1]; }
    if (cheaper) *cheaper = better ? 1 : 0;
    *num_records = (uint32_t)adapted.size();
    *entry_ref = entry;
    if (records)
    {
        if (adapted.size() > capacity) return fail(nullptr, "rt_debug_adapt_fold: capacity too small");
        memcpy(records, adapted.data(), adapted.size() * sizeof(WideNode));
        if (roots) memcpy(roots, adapted_roots.data(), adapted_roots.size() * sizeof(uint32_t));
    }
    return RT_OK;
}

// RT_CTX_OPT_ADAPTIVE_FOLD's trigger on its own: has camera `now` left the view the folds were adapted to (`adapted`), in a scene of this diagonal?
int rt_debug_fold_view_left(const rt_camera* adapted, const rt_camera* now, double scene_diagonal)
{
    if (!adapted || !now) return -1;
    FoldAdapt a;
    a.camera = *adapted;
    a.scene_diagonal = scene_diagonal;
    return fold_view_left(a, *now) ? 1 : 0;
}

// FoldAdapt's shadow side exactly as the worker runs it (adapt_shadow_side; host only): `nodes` is the shadow rays' current binary tree under its surface-area
// fold, `mode` RT_CTX_OPT_ADAPTIVE_FOLD's value (bit 3 = rotate first).  Out: the candidate's records, the tree they fold (out_tree[num_nodes]; `nodes`
// again when nothing was rotated), cost2 = {current, candidate}, *rotations, return value 1 = would be adopted, 0 = kept, < 0 = error.
int rt_debug_adapt_shadow_side(const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays, uint32_t mode,
    void* records, uint32_t* roots, uint32_t capacity, uint32_t* num_records, uint32_t* entry_ref, rt_bvh_node* out_tree, double* cost2, uint32_t* rotations,
    const rt_triangle* triangles, uint32_t num_triangles, uint32_t* reordered)
{
    if (!nodes || num_nodes == 0 || !origins_tmax || !directions || !num_records || !entry_ref) { fail(nullptr, "rt_debug_adapt_shadow_side: NULL argument"); return -1; }
    FoldAdapt a;
    a.mode = mode;
    if (triangles && (mode & 16u))
    {
        a.tri9.resize((size_t)num_triangles * 9);
        for (uint32_t i = 0; i < num_triangles; ++i)
        {
            const rt_float3 v[3] = {triangles[i].v1.position, triangles[i].v2.position, triangles[i].v3.position};
            for (int k = 0; k < 3; ++k) { a.tri9[(size_t)i * 9 + 3 * k] = v[k].x; a.tri9[(size_t)i * 9 + 3 * k + 1] = v[k].y; a.tri9[(size_t)i * 9 + 3 * k + 2] = v[k].z; }
        }
    }
    a.bvh2.assign(nodes, nodes + num_nodes);
    std::vector<WideNode> wide;
    uint32_t entry = 0;
    if (!build_wide_bvh(nodes, num_nodes, RT_WIDE_SAH, wide, entry, &a.roots) || wide.empty()) { fail(nullptr, "rt_debug_adapt_shadow_side: the tree does not qualify for the 4-wide layout"); return -1; }
    a.sh_o.resize(n_rays); a.sh_d.resize(n_rays);
    for (uint32_t i = 0; i < n_rays; ++i)
    {
        a.sh_o[i] = make_float4(origins_tmax[4 * i], origins_tmax[4 * i + 1], origins_tmax[4 * i + 2], origins_tmax[4 * i + 3]);
        a.sh_d[i] = make_float4(directions[4 * i], directions[4 * i + 1], directions[4 * i + 2], 0.0f);
    }
    const bool adopted = adapt_shadow_side(&a);
    if (a.wide_sh.empty()) { fail(nullptr, "rt_debug_adapt_shadow_side: no candidate (no ray passed the root box, or the folds are too deep)"); return -1; }
    *num_records = (uint32_t)a.wide_sh.size();
    *entry_ref = a.entry_sh;
    if (cost2) { cost2[0] = a.cost[1][0]; cost2[1] = a.cost[1][1]; }
    if (rotations) *rotations = a.rotations;
    if (reordered) *reordered = a.reordered;
    if (records)
    {
        if (a.wide_sh.size() > capacity) { fail(nullptr, "rt_debug_adapt_shadow_side: capacity too small"); return -1; }
        memcpy(records, a.wide_sh.data(), a.wide_sh.size() * sizeof(WideNode));
        if (roots) memcpy(roots, a.roots_sh_new.data(), a.roots_sh_new.size() * sizeof(uint32_t));
    }
    if (out_tree) memcpy(out_tree, a.rotations != 0 ? a.bvh2_sh_new.data() : nodes, (size_t)num_nodes * sizeof(rt_bvh_node));
    return adopted ? 1 : 0;
}

// What rt_scene_upload / rt_ctx_destroy do to an adaptation in flight (host only): a FoldAdapt whose worker has just started on `nodes` and the rays
// given is dropped after delay_ms; returns the milliseconds the drop took (the worker gives up at its next check), -1 on an argument error.
double rt_debug_fold_abandon(const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays, uint32_t mode,
    uint32_t delay_ms, int* had_finished)
{
    if (!nodes || num_nodes == 0 || !origins_tmax || !directions) { fail(nullptr, "rt_debug_fold_abandon: NULL argument"); return -1.0; }
    FoldAdapt* a = new FoldAdapt();
    a->mode = mode;
    a->bvh2.assign(nodes, nodes + num_nodes);
    std::vector<WideNode> wide;
    uint32_t entry = 0;
    if (!build_wide_bvh(nodes, num_nodes, RT_WIDE_SAH, wide, entry, &a->roots) || wide.empty()) { delete a; fail(nullptr, "rt_debug_fold_abandon: the tree does not qualify"); return -1.0; }
    a->o.resize(n_rays); a->d.resize(n_rays);
    for (uint32_t i = 0; i < n_rays; ++i)
    {
        a->o[i] = make_float4(origins_tmax[4 * i], origins_tmax[4 * i + 1], origins_tmax[4 * i + 2], origins_tmax[4 * i + 3]);
        a->d[i] = make_float4(directions[4 * i], directions[4 * i + 1], directions[4 * i + 2], 0.0f);
    }
    a->sh_o = a->o; a->sh_d = a->d;
    a->state = FoldAdapt::COMPUTING;
    a->worker = std::thread(fold_adapt_worker, a);
    std::this_thread::sleep_for(std::chrono::milliseconds(delay_ms));
    if (had_finished) *had_finished = a->finished.load() ? 1 : 0;
    const auto t0 = std::chrono::steady_clock::now();
    drop_fold_adapt(a);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// tree_rotate.h on its own (host only): the binary tree `nodes` rotated for the rays given (as rt_debug_adapt_fold takes them); out_nodes[num_nodes]
int rt_debug_rotate_tree(const rt_bvh_node* nodes, uint32_t num_nodes, const float* origins_tmax, const float* directions, uint32_t n_rays, int max_passes,
    rt_bvh_node* out_nodes, double* cost2, uint32_t* rotations, int moves, double min_gain)
{
    if (!nodes || num_nodes == 0 || !origins_tmax || !directions || !out_nodes) return fail(nullptr, "rt_debug_rotate_tree: NULL argument");
    std::vector<rt_bvh_node> out;
    double cost[2] = {0.0, 0.0};
    const uint32_t made = treerot::rotate(nodes, num_nodes, origins_tmax, directions, n_rays, max_passes, out, cost, nullptr, moves, min_gain);
    if (out.size() != num_nodes) return fail(nullptr, "rt_debug_rotate_tree: the node array is not a tree");
    memcpy(out_nodes, out.data(), out.size() * sizeof(rt_bvh_node));
    if (cost2) { cost2[0] = cost[0]; cost2[1] = cost[1]; }
    if (rotations) *rotations = made;
    return RT_OK;
}

} // extern "C"
