// tile_shard.cpp -- see include/volrend/internal/tile_shard.hpp.
#include "volrend/internal/tile_shard.hpp"

#include <cstdlib>
#include <stdexcept>

#include "volrend/internal/check.hpp"

namespace volrend {
namespace internal {
namespace {

void gather_ok(int rc, const char* what) {  // libvolrend_gather: the shard's RCCL collective
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + vr_gather_last_error());
}

}  // namespace

TileShardRenderer::TileShardRenderer(const N3Tree& tree, int width, int height,
                                     const TileShardConfig& cfg)
    : n_(cfg.n_ranks < 1 ? 1 : cfg.n_ranks),
      width_(width),
      height_(height),
      tile_w_((width + 7) / 8 * 8),
      tile_h_(cfg.tile_rows < 8 ? 8 : cfg.tile_rows / 8 * 8),
      max_batch_(cfg.max_batch < 1 ? 1 : (cfg.max_batch > VR_MAX_BATCH ? VR_MAX_BATCH : cfg.max_batch)),
      share_(cfg.share_device && n_ > 1),
      rccl_self_(n_ == 1),
      ranks_((size_t)n_) {
    // (a throw below frees what has been built so far through the members)
    if (!tree.device) throw std::runtime_error("TileShardRenderer: the tree is not on a device");
    int n_dev = 0;
    hip_check(hipGetDeviceCount(&n_dev), "hipGetDeviceCount");
    for (int r = 0; r < n_; ++r) ranks_[r].device = share_ ? cfg.first_device : cfg.first_device + r;
    if (cfg.first_device < 0 || ranks_.back().device >= n_dev)
        throw std::runtime_error("TileShardRenderer: " + std::to_string(n_) + " ranks from device " +
                                 std::to_string(cfg.first_device) + " need more GPUs than the " +
                                 std::to_string(n_dev) + " visible (--share_gpu rehearses on one)");
    compact_bytes_ = vr_compact_bytes(width_, height_, tile_w_, tile_h_, n_);
    if (compact_bytes_ <= 0) throw std::runtime_error("TileShardRenderer: bad tile geometry");
    const int root = ranks_[0].device;

    // The gather sends every peer's tiles straight to the root GPU: that needs peer access
    // (xGMI inside a node) between the root and each peer.  Without it RCCL falls back to
    // staging through host memory -- correct but no longer the path this class exists for --
    // so say so loudly instead of silently running 10x slower.  VOLREND_ALLOW_NO_P2P=1 proceeds.
    std::string p2p_note;
    if (!share_) {
        std::string no_p2p;
        for (int r = 1; r < n_; ++r) {
            int to_root = 0, from_root = 0;
            hip_check(hipDeviceCanAccessPeer(&to_root, ranks_[r].device, root), "hipDeviceCanAccessPeer");
            hip_check(hipDeviceCanAccessPeer(&from_root, root, ranks_[r].device), "hipDeviceCanAccessPeer");
            if (!to_root || !from_root) no_p2p += " " + std::to_string(ranks_[r].device);
        }
        const char* allow = getenv("VOLREND_ALLOW_NO_P2P");
        if (!no_p2p.empty() && !(allow && allow[0] == '1'))
            throw std::runtime_error(
                "TileShardRenderer: no peer access between the root GPU " + std::to_string(root) +
                " and GPU(s)" + no_p2p + " (hipDeviceCanAccessPeer = 0): the RGBA8 gather and the "
                "tree replicas would be staged through host memory.  Check `rocm-smi --showtopo`, "
                "IOMMU / ACS settings and HSA_ENABLE_IPC_MODE_LEGACY=0; set VOLREND_ALLOW_NO_P2P=1 to "
                "run anyway, or --share_gpu to rehearse on one device");
        p2p_note = no_p2p.empty() ? "peer access to the root: yes"
                                  : "NO peer access for GPU(s)" + no_p2p + " (host-staged)";
    }
    VrTreeInfo info;
    vr_check(vr_tree_info(tree.device, &info), "vr_tree_info");
    for (int r = 0; r < n_; ++r) {
        Rank& k = ranks_[r];
        DeviceGuard on(k.device);
        // one replica per rank; the caller's copy serves the root when it already lives there
        if (r == 0 && info.device == root) {
            k.tree = tree.device;
        } else {
            vr_check(vr_tree_clone(tree.device, k.device, &k.tree), "vr_tree_clone");
            k.clone.reset(k.tree);
        }
        // the rank's tiles, rounded up to whole tiles, one slot (one render stream per rank)
        vr_check(vr_reserve_tiles(k.tree, width_, height_, max_batch_, tile_w_, tile_h_, n_, 1),
                 "vr_reserve_tiles");
        hip_check(k.render_stream.create(hipStreamNonBlocking), "DeviceStream::create");
        hip_check(k.comm_stream.create(hipStreamNonBlocking), "DeviceStream::create");
        for (int s = 0; s < 2; ++s) {
            hip_check(k.rendered[s].create(), "DeviceEvent::create");
            hip_check(k.released[s].create(), "DeviceEvent::create");
            if (r > 0 || rccl_self_)
                hip_check(k.compact[s].alloc((size_t)compact_bytes_ * max_batch_),
                          "DeviceBuffer::alloc(compact)");
        }
    }
    DeviceGuard on(root);
    for (int s = 0; s < 2; ++s) {
        hip_check(gather_[s].alloc((size_t)compact_bytes_ * max_batch_ * n_), "DeviceBuffer::alloc(gather)");
        hip_check(frames_[s].alloc(frame_bytes() * max_batch_), "DeviceBuffer::alloc(frames)");
    }
    if (!share_) {
        std::vector<int> devices;
        for (const Rank& k : ranks_) devices.push_back(k.device);
        std::vector<vr_gather_t> comms((size_t)n_, nullptr);
        gather_ok(vr_gather_init_all(n_, devices.data(), comms.data()), "vr_gather_init_all");
        for (int r = 0; r < n_; ++r) ranks_[r].gather.reset(comms[r]);
        transport_ = "RCCL " + std::to_string(vr_gather_version()) + ", " + std::to_string(n_) +
                     (n_ == 1 ? " rank (self send/recv)" : " ranks, grouped send/recv to the root") +
                     (n_ > 1 ? ", " + p2p_note : "");
    } else {
        transport_ = "REHEARSAL: " + std::to_string(n_) + " ranks share device " +
                     std::to_string(root) + ", tiles move with hipMemcpyAsync (no RCCL)";
    }
}

TileShardRenderer::~TileShardRenderer() {
    // every rank's work is done before anything goes, and the RCCL communicators go before the
    // streams and buffers they use; the members free the rest, each on its own device
    for (const Rank& k : ranks_) {
        DeviceGuard on(k.device);
        (void)hipDeviceSynchronize();
    }
    for (Rank& k : ranks_) k.gather.reset();
}

void TileShardRenderer::render(int seq, const VrCamera* cams, int n, const VrRenderOptions& opt,
                               int fp_mode) {
    if (n < 1 || n > max_batch_) throw std::invalid_argument("TileShardRenderer::render: batch size");
    const int s = seq & 1;
    const size_t share = (size_t)compact_bytes_;
    const size_t rank_stride = share * max_batch_;
    Rank& root = ranks_[0];
    std::vector<VrFrame> frames((size_t)n);
    // 1. every rank renders its tiles of the n poses into its COMPACT buffer of set s
    for (int r = 0; r < n_; ++r) {
        Rank& k = ranks_[r];
        DeviceGuard on(k.device);
        uint8_t* dst = (r == 0 && !rccl_self_) ? gather_[s].get<uint8_t>() : k.compact[s].get<uint8_t>();
        // set s is free again once the transfer (root: the assembly) of launch seq - 2 is done
        if (k.released_used[s])
            hip_check(hipStreamWaitEvent(k.render_stream.get(), k.released[s].get(), 0), "hipStreamWaitEvent");
        for (int i = 0; i < n; ++i) {
            vr_default_frame(&frames[i]);
            frames[i].rgba = dst + share * i;
            frames[i].offscreen = 1;
            frames[i].layout = VR_LAYOUT_COMPACT;
            frames[i].tile_w = tile_w_;
            frames[i].tile_h = tile_h_;
            frames[i].rank = r;
            frames[i].world = n_;
            frames[i].fp_mode = fp_mode;
        }
        vr_check(vr_render_batch(k.tree, n, cams, &opt, frames.data(), k.render_stream.get()),
                 "vr_render_batch");
        hip_check(hipEventRecord(k.rendered[s].get(), k.render_stream.get()), "hipEventRecord");
        hip_check(hipStreamWaitEvent(k.comm_stream.get(), k.rendered[s].get(), 0), "hipStreamWaitEvent");
    }
    // 2. the tiles travel to the root: rank r's n shares land at gather + r * rank_stride
    if (!share_) {
        // (the same entry point bench.py --gpus N drives, one rank per process there: include/volrend_gather.h)
        gather_ok(vr_gather_group_begin(), "vr_gather_group_begin");
        for (Rank& k : ranks_)
            gather_ok(vr_gather_tiles(k.gather.get(), k.compact[s].get(), gather_[s].get(), (int64_t)rank_stride,
                                      (int64_t)(share * n), rccl_self_ ? 1 : 0, k.comm_stream.get()),
                      "vr_gather_tiles");
        gather_ok(vr_gather_group_end(), "vr_gather_group_end");
    } else {
        DeviceGuard on(root.device);
        for (int r = 1; r < n_; ++r) {
            // same device: the root's communication stream copies once rank r has rendered
            hip_check(hipStreamWaitEvent(root.comm_stream.get(), ranks_[r].rendered[s].get(), 0),
                      "hipStreamWaitEvent");
            hip_check(hipMemcpyAsync(gather_[s].get<uint8_t>() + rank_stride * r, ranks_[r].compact[s].get(),
                                     share * n, hipMemcpyDeviceToDevice, root.comm_stream.get()),
                      "hipMemcpyAsync");
        }
    }
    // 3. the root de-interleaves the batch; 4. the buffers of set s are released
    {
        DeviceGuard on(root.device);
        vr_check(vr_assemble_tiles_batch(frames_[s].get(), (int64_t)frame_bytes(), 0, gather_[s].get(),
                                         (int64_t)rank_stride, (int64_t)share, n, width_, height_, tile_w_,
                                         tile_h_, n_, root.comm_stream.get()),
                 "vr_assemble_tiles_batch");
    }
    for (Rank& k : ranks_) {
        DeviceGuard on(k.device);
        // shared device: rank r's buffer is read by the ROOT's stream
        const DeviceStream& after = share_ ? root.comm_stream : k.comm_stream;
        hip_check(hipEventRecord(k.released[s].get(), after.get()), "hipEventRecord");
        k.released_used[s] = true;
    }
}

void TileShardRenderer::sync() {
    for (const Rank& k : ranks_) {
        DeviceGuard on(k.device);
        hip_check(hipStreamSynchronize(k.render_stream.get()), "hipStreamSynchronize");
        hip_check(hipStreamSynchronize(k.comm_stream.get()), "hipStreamSynchronize");
    }
    // every launch has run: a rank whose rays hit the sample guard rendered wrong tiles.  ALL ranks'
    // words are read and cleared before anything is thrown -- a later sync() must not trip over
    // stale bits of these launches
    std::string failed;
    for (int r = 0; r < n_; ++r) {
        uint32_t status = 0;
        vr_check(vr_tree_status(ranks_[r].tree, &status, 1), "vr_tree_status");
        if (status != 0)
            failed += (failed.empty() ? "" : ", ") + std::to_string(r) + " (0x" + std::to_string(status) + ")";
    }
    if (!failed.empty())
        throw std::runtime_error("tile shard: render status of rank(s) " + failed +
                                 " (rays hit the sample guard: step_size too small for this scene?); "
                                 "the frames are wrong");
}

}  // namespace internal
}  // namespace volrend
