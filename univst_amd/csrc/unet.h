// UNet handle internals (see unet.hip).
#pragma once
#include <memory>
#include <string>
#include <unordered_map>

#include "../../include/univst.h"
#include "model.h"
#include "motion.h"

struct UNet : Model {
    univst_unet_cfg cfg;
    std::unordered_map<long, int*> idx_tables;
    std::unordered_map<std::string, long> temb_off;    // resnet prefix -> column offset in the fused time_emb_proj (finalize)
    long temb_total = 0;
    // The tuning switches: the DEFAULTS live here, names / environment seeds / accepted ranges in the option table of abi.hip (kUNetOptions)
    int gn_producer = 1;      // GroupNorm statistics from the producing conv / linear's epilogue where the tile geometry allows (0: always the stand-alone pass)
    int chain_bands = 1;      // post-attention chain of a transformer block in row bands: 1 off (default: measured +0.4 ms per step in the graph), 0 auto (bands of >= 65536 rows), n > 1 forced
    int gn_fold = 1;          // the transformer blocks' per-frame GroupNorm folded into proj_in where the weight copies are cheap (round 5; 0: the apply pass)
    int attn2_fused = 2;      // the text cross-attention of a block as one launch where fused.hip serves the shape (round 5): 2 = with the self-attention's out projection in front, 1 = attn2 alone, 0 = q projection + attention + out projection
    int ln_fold = 2;          // transformer-block LayerNorms folded into the neighbouring linears: 0 none, 1 norm1 + norm2, 2 also norm3 (default since round 4)
    int kcat_fold = 3;        // bit 0: proj_out as extra K columns of ff.net.2 — one K = 5C GEMM over the channel concat [mid | h3] with the composed weight "proj_out#kcat" (finalize) instead of two launches; bit 1: reserved for conv_shortcut as a tail of conv2, NOT BUILT (the graph launches the shortcut separately whatever the bit says)
    // AnimateDiff UNet3D (univst_unet_create_animatediff): the per-frame 2-D graph with a motion module behind every resnet / transformer pair.
    // The modules keep their own weight stores (keys below "<block>.motion_modules.<j>."); their chains run on THIS handle's arena and split-K workspace.
    bool animatediff = false;
    univst_animatediff_cfg ad = {};
    std::unordered_map<std::string, std::unique_ptr<Motion>> motions;     // "down_blocks.0.motion_modules.1" -> module (created by create, every configured slot)
    std::unordered_map<std::string, int> motion_active;                   // the modules whose proj_out is not all zeros (found on the device at finalize)
    int motion_fold = 0;      // reserved: the module's GroupNorm / LayerNorms folded into the neighbouring GEMMs — NOT BUILT (set_option refuses 1)
    unsigned* d_counter = nullptr;
    // TRAINED temporal layers (fine-tuned 3-D checkpoints): the units whose *_temporal* parameters differ from the identity
    // initialisation (found on the device at finalize).  Empty for 2-D-initialised weights: the graph then skips them exactly.
    std::unordered_map<std::string, int> temporal_conv_active;     // conv prefix ("...resnets.0.conv1", "conv_in", ...)
    std::unordered_map<std::string, int> temporal_attn_active;     // transformer block prefix ("...transformer_blocks.0")
    // multi-GPU frame sharding hooks
    int rank = 0, world = 1;
    univst_allreduce_fn allreduce = nullptr;
    univst_kv_exchange_fn kv_exchange = nullptr;
    void* comm_user = nullptr;
    char* comm_ws = nullptr;
    long comm_ws_bytes = 0;
    struct univst_comm* native_comm = nullptr;   // set when the hooks above are the library's own IPC communicator (comm.hip)
    // round 6: the K/V exchange of a transformer block runs on a FORKED stream beside the block's own q|k|v projection and the local phase of its
    // attention (Fwd::kv_post / kv_join); kv_overlap = 0 issues it on the forward's stream instead (A/B aid).  emu_wire_*: bench.py --emulate-wire —
    // with a communicator that moves nothing (NullComm) a delay kernel on the forked stream stands in for the slowest transfer of each exchange.
    int kv_overlap = 1;
    int emu_wire_gbps = 0, emu_wire_lat_us = 3;
    double emu_wire_us = 0.0;                    // modelled wire time issued since the last univst_unet_query("emu_wire_us")
    hipStream_t xstream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool x_dirty = false;                        // the forked stream carries work of this forward that the forward's stream has not joined yet
    unsigned* emu_flag = nullptr;                // [0] the emulated inbox flag (device), [1] a status word for the wait kernel
    unsigned emu_epoch = 0;
    int comm_streams();                          // creates the forked stream + events on first use

    // Static style (include/univst.h univst_unet_style_bank): the style branch of the PnP step as ONE frame.  The bank is caller-owned device memory that
    // holds, per PnP layer in graph order, the K | V rows [N_l, 2 C_l] fp16 of that frame, each layer's block starting on a 256-byte boundary.
    struct StyleBank {
        enum { WRITE = 1, READ = 2 };
        int mode = 0;              // WRITE: the one-frame forward leaves its K | V rows and stops behind the last PnP layer; READ: the B = 2 forward shifts against them
        char* base = nullptr;
    };
    std::vector<long> style_bank_layout(int H, int W) const;       // byte offset of every PnP layer's block, then the total
    int static_style_check(const char* entry) const;                 // the handles the static style is refused on (UV_ERR_UNSUPPORTED), by name

    UNet() : Model("unet") {}
    ~UNet();
    int load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s);
    int finalize(hipStream_t s);
    int reserve(int B, int F, int H, int W);
    int forward(const half_t* sample, float timestep, const half_t* text, int B, int F, int H, int W, int text_len,
                const univst_pnp* pnp, half_t* eps_out, half_t* feat_out, int ft_index, hipStream_t s, bool tap_entry = false,
                const StyleBank* bank = nullptr);
    static bool pnp_window_active(bool animatediff, const univst_pnp* pnp);      // registered and idx inside the shift window of that backbone
};
