/* univst.h — C ABI of libunivst_hip.so: the MI355X (gfx950) implementation of the UniVST SD-v1.5
 * denoising hot path.  Plain pointers and sizes only; no torch types.  All pointers are DEVICE pointers
 * unless stated otherwise; all tensors are fp16 (IEEE binary16) unless stated otherwise; all work is
 * enqueued on the caller-supplied hipStream_t (passed as void*) and the call returns without syncing.
 *
 * Every entry returns 0 on success or a negative code (UNIVST_ERR_*); the message is available through
 * univst_last_error() (thread-local).  Handles are not re-entrant: one call at a time per handle.
 *
 * The reference (QuanjianSong/UniVST) is pure Python with no native layer, so there is no existing FFI to
 * mimic; each entry names the reference interface (file:line under the reference checkout) it replaces.
 * The Python binding a maintainer adds is univst_amd/_native.py (ctypes); see INTEGRATION.md.
 */
#ifndef UNIVST_H
#define UNIVST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define UNIVST_OK 0
#define UNIVST_ERR_ARG (-1)
#define UNIVST_ERR_HIP (-2)
#define UNIVST_ERR_UNSUPPORTED (-3)
#define UNIVST_ERR_STATE (-4)

#define UNIVST_F16 0
#define UNIVST_F32 1

const char* univst_last_error(void);
/* Bumped whenever an existing entry changes its signature or meaning (2: univst_sd3_joint_attention takes (shift, beta) instead of the
 * window parameters, round 4).  A binding checks it at load time (univst_amd/_native.py does): a caller built against an older header would
 * otherwise pass silently misinterpreted arguments. */
#define UNIVST_ABI_VERSION 3
int univst_abi_version(void);

/* ------------------------------------------------------------------ UNet handle
 * Replaces backbones/video_diffusion_sd/models/unet_3d_condition.py:49-230 (ctor), :306-443 (forward),
 * :445-509 (from_2d_model / load_2d_state_dict). */
typedef struct univst_unet univst_unet;

typedef struct {
    int in_channels, out_channels;
    int block_out_channels[4];
    int layers_per_block;
    int cross_attention_dim;
    int attention_heads[4];     /* SD config key attention_head_dim per down level, used as HEAD COUNT (unet_3d_blocks.py:269-271);
                                   SD-v1.x: 8,8,8,8 (head_dim = C/8); SD-v2.x: 5,10,20,20 (head_dim 64) */
    int norm_num_groups;
    float norm_eps;
    int flip_sin_to_cos;
    float freq_shift;
} univst_unet_cfg;

/* PnP state = what register_spatial_attention_pnp / register_time (pnp_utils.py:7-111) poke into attn1. */
typedef struct {
    int registered;             /* 1: the 8 decoder attn1 layers use the PnP forward ([-1,'first'] K/V sources) */
    int idx;                    /* step index (register_time) */
    float eta1, eta2;           /* window: eta1 <= idx <= eta2*50 */
    float alpha, gamma;         /* 0.65, 3.0 (pnp_utils.py:49-51) */
} univst_pnp;

int univst_unet_create(const univst_unet_cfg* cfg, univst_unet** out);
int univst_unet_destroy(univst_unet* h);
/* key = reference state-dict name (incl. *_temporal*); data is copied (D2D) and converted to fp16 */
int univst_unet_load_tensor(univst_unet* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape,
                            int ndim, void* stream);
/* builds the derived weight layouts ([Cout][ky][kx][Cin] convs, fused QKV / KV, GEGLU-interleaved FF) and
 * inspects the *_temporal* layers on the device: units still at their identity initialisation (dirac conv1d, zero
 * attn_temporal.to_out: every 2-D-initialised checkpoint) are skipped exactly; TRAINED units (a fine-tuned 3-D checkpoint) get their
 * derived layouts and run (resnet.py:70-80 as a 3-tap conv over frames through the conv kernels, attention.py:336-346 in a frame
 * attention kernel).  Trained temporal layers and frame sharding exclude each other (forward returns UNIVST_ERR_ARG). */
int univst_unet_finalize(univst_unet* h, void* stream);
/* (re)allocates the activation arena for this geometry; forward() calls it implicitly on first use */
int univst_unet_reserve(univst_unet* h, int B, int F, int H, int W);
/* sample [B,Cin,F,H,W], text [B,77,Dtxt] -> eps [B,Cout,F,H,W].  feat_out (may be NULL): receives the output
 * of up_blocks[ft_index] for batch element 0 as [F,H',W',C] (unet_3d_condition.py:430-436). */
int univst_unet_forward(univst_unet* h, const void* sample, float timestep, const void* text, int B, int F, int H,
                        int W, int text_len, const univst_pnp* pnp, void* eps_out, void* feat_out, int ft_index,
                        void* stream);
/* univst_unet_forward plus the feature tap on every kind of handle: feat_out receives the output of up_blocks[ft_index] (after its upsampler)
 * for batch element 0 as [F,H',W',C] fp16 (animatediff/models/unet.py:453-459).  feat_out NULL or ft_index outside 0..3: UNIVST_ERR_ARG before any launch. */
int univst_unet_forward_tap(univst_unet* h, const void* sample, float timestep, const void* text, int B, int F, int H, int W, int text_len,
                            const univst_pnp* pnp, void* eps_out, void* feat_out, int ft_index, void* stream);
/* Static style: the style branch of the PnP step as ONE frame instead of F copies of it (DESIGN.md "Static style branch").  The style input of
 * the SD path is a single image repeated F times (ddim_inversion.py:45-65); with 2-D-initialised temporal layers F identical frames give F identical
 * results, and all the stylised branch takes from the style branch is the to_k / to_v rows of the same frame at the eight PnP layers
 * (pnp_utils.py:54-55).  A step inside the window is then two calls: univst_unet_style_bank (one frame, B = F = 1) fills the bank, and
 * univst_unet_forward_static_style (B = 2: content, stylised) shifts against it.
 *
 * The bank is caller-owned device memory, 16-byte aligned, of univst_unet_style_bank_bytes(h, H, W) bytes (a negative code on a bad argument).  Layout:
 * for each PnP layer in graph order (up_blocks.1.attentions.1, .2, up_blocks.2.attentions.0 .. 2, up_blocks.3.attentions.0 .. 2) the K | V rows
 * [N_l, 2 C_l] fp16 of the style frame (N_l = that level's H' * W', row stride 2 C_l, K columns first), each layer's block starting at a multiple of
 * 256 bytes.  The column statistics of the shift are NOT kept in the bank: the shift takes them from the rows (one frame) on every call.
 *
 *   style_bank            sample [1,Cin,1,H,W], text [1,L,D].  Runs the frame with the PnP key sources and WITHOUT the shift (the reference only ever
 *                         modifies chunk 2, pnp_utils.py:53-57) up to the last PnP layer's projection, leaving every layer's rows in the bank.
 *                         *active_out = whether pnp->idx is inside the window; outside it the call returns UNIVST_OK without a launch and
 *                         leaves the bank alone.  pnp NULL or not registered, a NULL bank with the window open, bank_bytes too small: UNIVST_ERR_ARG.
 *   forward_static_style  sample [2,Cin,F,H,W] (content, stylised), text [2,L,D] -> eps [2,Cout,F,H,W].  Inside the window the eight PnP layers
 *                         run univst_attention_adain_shift_static against the bank; a NULL or too small bank there is UNIVST_ERR_ARG.  Outside the
 *                         window (or with pnp NULL / not registered) it is exactly univst_unet_forward with B = 2, and bank may be NULL.
 * Refused with UNIVST_ERR_UNSUPPORTED before any launch, both entries: a handle of univst_unet_create_animatediff (the motion modules' position
 * encoding makes identical frames differ), a handle on which finalize found a trained temporal unit (the frames are coupled), a handle with a
 * communicator attached (the halo phase of a frame shard shifts against the style's hidden rows). */
int64_t univst_unet_style_bank_bytes(univst_unet* h, int H, int W);
int univst_unet_style_bank(univst_unet* h, const void* sample, float timestep, const void* text, int H, int W, int text_len, const univst_pnp* pnp,
                           void* bank, int64_t bank_bytes, int* active_out, void* stream);
int univst_unet_forward_static_style(univst_unet* h, const void* sample, float timestep, const void* text, int F, int H, int W, int text_len,
                                     const univst_pnp* pnp, const void* bank, int64_t bank_bytes, void* eps_out, void* stream);
/* frame-sharded multi-GPU: this rank holds frames [rank*F, (rank+1)*F) of a clip of world*F frames
 * for ALL branches.  comm_ws is a caller-owned device workspace (>= 64 KiB + 4 x the largest frame pack); the callbacks are invoked on the
 * host while forward() enqueues work and must enqueue the collective on the SAME stream forward() was given (RCCL through
 * torch.distributed on the Python side):
 *   allreduce(user, byte_off, n)         : in-place SUM over ranks of n fp32 at comm_ws + byte_off  (5-D GroupNorm)
 *   kv_exchange(user, off_send_last, off_first, off_recv_prev, off_recv_first, nbytes):
 *        rank 0 broadcasts [off_first, +nbytes) (others receive it at off_recv_first); every rank r < world-1
 *        sends [off_send_last, +nbytes) to r+1, every rank r > 0 receives it at off_recv_prev  (sparse-causal attention, attention.py:384-413).
 * ABI 3 (round 6): a pack is the transformer block's HIDDEN rows of the boundary frame of every branch, [B, N, C] fp16 (the input of norm1 ->
 * to_k | to_v; until ABI 2: the K | V rows, [B, N, 2C]); the receiving rank projects (and, inside the PnP window, shifts) the two halo frames
 * itself and runs the attention in two phases (univst_attention_phase).  The callback only moves bytes and is invoked between the phases. */
typedef int (*univst_allreduce_fn)(void* user, int64_t byte_off, int count_f32);
typedef int (*univst_kv_exchange_fn)(void* user, int64_t off_send_last, int64_t off_first, int64_t off_recv_prev,
                                     int64_t off_recv_first, int64_t nbytes);
int univst_unet_set_comm(univst_unet* h, int rank, int world, void* comm_ws, int64_t comm_ws_bytes,
                         univst_allreduce_fn ar, univst_kv_exchange_fn kv, void* user);

/* The library's own frame-shard communicator (csrc/comm.hip): one process per GPU of ONE node, peers' regions mapped
 * through HIP IPC, all three couplings (GroupNorm statistics all-reduce, K/V halo + first-frame broadcast, latent_adain statistics)
 * as device-side peer writes + flags on the caller's stream — no host callbacks, so a forward() is a pure stream of kernels.
 * Replaces what the reference would need for `attention.py:384-413` / the 5-D GroupNorms of `resnet.py:338,369` across GPUs (the
 * reference itself is single-GPU).  Bring-up sequence on every rank:
 *   univst_comm_create(rank, world, ws_bytes, &c)      ws_bytes >= 64 KiB + 6 x the largest frame pack (B*N*C fp16 of hidden rows; B*N*2C keeps room for the SD3 K | V packs)
 *   univst_comm_export(c, handle)                      univst_comm_handle_bytes() bytes, to be all-gathered out of band
 *   univst_comm_connect(c, all_handles)                rank-major array of every rank's handle
 *   univst_unet_set_comm_native(unet, c)               the UNet graph now uses it instead of callbacks
 * Every wait is bounded; a rank that gives up records a code (univst_comm_status) and the next call returns UNIVST_ERR_STATE. */
typedef struct univst_comm univst_comm;
int univst_comm_create(int rank, int world, int64_t ws_bytes, univst_comm** out);
int univst_comm_handle_bytes(void);
int univst_comm_export(univst_comm* c, void* handle_out);
int univst_comm_connect(univst_comm* c, const void* handles);
/* ranks that are host threads of ONE process (tests on a 1-GPU box): `all` = the `world` communicators in rank order */
int univst_comm_connect_local(univst_comm* c, univst_comm* const* all);
/* ONE rank of a `world`-rank job alone on one GPU (bench.py --emulate-rank r/w --comm-emulated; measurement aid, results are meaningless): every peer
 * is this rank's own region; an exchange's post becomes a delay of latency + (packs on this rank's busiest link) x bytes / link rate followed by a
 * raise of its own inbox flags, on the stream the multicast would run on; an all-reduce runs over this rank alone after `latency_us`.  Kernels, streams
 * and flag waits are the production ones.  univst_comm_query("emu_wire_us"): the modelled time issued since the last query. */
int univst_comm_connect_emulated(univst_comm* c, double link_gbps, double latency_us);
int univst_comm_query(univst_comm* c, const char* name, double* out);
int univst_comm_destroy(univst_comm* c);
/* in-place SUM over ranks of n <= 1024 fp32 in device memory, identical bits on every rank (slots summed in rank order) */
int univst_comm_allreduce_f32(univst_comm* c, void* buf, int n, void* stream);
int univst_comm_status(univst_comm* c);
int univst_unet_set_comm_native(univst_unet* h, univst_comm* comm);

/* tuning switches of a handle (not part of the reference's surface; tests use them for A/B runs).  The library keeps ONE table of them (abi.hip: name,
 * environment seed, accepted range): univst_unet_create seeds a new handle from the environment — a seed is clamped into the range, never refused;
 * UNIVST_CHAIN_BANDS alone has no upper clamp — univst_unet_set_option refuses a value outside the range with UV_ERR_ARG and leaves the option as it
 * was (the 0 / 1 switches gn_producer, gn_fold and kv_overlap take any int as != 0), and univst_unet_query("<option name>") reads the current value back.
 *   "ln_fold" (default 2 since round 4, env UNIVST_LN_FOLD): fold the transformer blocks' LayerNorms (attention.py:311,321,329) into the
 *             linears around them instead of launching them separately: 0 none, 1 norm1 + norm2, 2 also norm3 (-> GEGLU).
 *   "gn_producer" (default 1, env UNIVST_GN_PRODUCER): GroupNorm statistics (resnet.py:338,369, attention.py:121) are taken from the epilogue
 *             of the conv / linear that writes the tensor instead of a separate pass over it, wherever that kernel is the 256x320 tile
 *             (0: always the stand-alone pass; results differ by fp32 summation order only).
 *   "chain_bands" (default 1 = off, env UNIVST_CHAIN_BANDS): the row-local chain behind a transformer block's self-attention
 *             (to_out -> attn2 -> to_out -> GEGLU feed-forward, attention.py:316-329) runs band by band over whole frames so that a band's
 *             intermediates stay in the 256 MB Infinity Cache: 0 = auto (bands of >= 65 536 rows), n = n bands.  Same results up to fp32
 *             summation order (a band may take another tile than the full tensor).  An
 *             experiment kept as a switch: -13 % on the isolated chain (tools/bench_mall_bands.py), +0.4 ms per step in the graph.
 *   "gn_fold" (default 1, env UNIVST_GN_FOLD): the per-frame GroupNorm in front of a transformer block (attention.py:121) is folded into proj_in as per-frame
 *             weight sets + an fp32 bias where the copies are cheap against the apply pass they replace (the 64x64 level); 0: always the apply pass.
 *   "attn2_fused" (default 2, env UNIVST_ATTN2_PRE=0 -> 1): the text cross-attention of a transformer block (attention.py:321-327)
 *             as one launch (univst_attn2_fused) where the level's shape is served, instead of q projection + attention + out projection; 2 (default): with the
 *             self-attention's out projection + residual in front of it (univst_attn12_fused), 1: attn2 alone, 0: off.
 *   "kv_overlap" (default 1, env UNIVST_KV_OVERLAP; round 6): the frame shard's K/V exchange of a transformer block (attention.py:384-413 across GPUs)
 *             is issued on a forked stream as soon as proj_in has written the boundary frames' hidden rows and joined in front of the halo phase of
 *             the two-phase attention; 0: issued on the forward's own stream (serial; A/B aid).  Results are identical.
 *   "emu_wire_gbps" / "emu_wire_lat_us" (default 0 = off / 3; bench.py --emulate-wire): with a callback communicator that moves nothing, every
 *             exchange occupies the forked stream for latency + (packs on this rank's busiest link) x pack bytes / rate — a 1-GPU box's stand-in for
 *             the xGMI transfer; the accumulated time is univst_unet_query("emu_wire_us").
 *   "kcat_fold" (default 3, env UNIVST_KCAT_FOLD): linear maps that only add into, or chain onto, a neighbouring GEMM run as extra K columns of it.
 *             Bit 0 (value 1): proj_out of a spatial transformer (attention.py:151) rides behind the block's second feed-forward linear: one GEMM
 *             [mid | h3] x [Wp W2 | Wp]^T with K = 5C over the two buffers (a 1x1 conv over their channel concat; weights composed at finalize,
 *             univst_linear_compose) instead of ff.net.2 + residual followed by proj_out + residual; blocks with a trained temporal attention and banded
 *             chains keep the two launches.  Bit 1 (value 2): reserved for a resnet's conv_shortcut as a one-tap tail of conv2 — NOT BUILT: the value is
 *             accepted and the shortcut is launched separately, so 2 runs the graph of 0 and 3 the graph of 1.  0: the two launches everywhere.
 *             Results differ by fp16 rounding only (one rounding per composed weight instead of one per element of the intermediate tensor). */
int univst_unet_set_option(univst_unet* h, const char* name, int value);
/* read-outs of a handle.  Every *_query below answers "arena_high_water" (bytes), "arena_bytes" (the size of the activation slab: it changes only when
 * a reserve / forward had to replace it by a larger one) and "weight_bytes" (loaded tensors plus the copies finalize derives; a UNet's own store, without
 * its motion modules').  This one adds "emu_wire_us" (modelled wire time issued since the last query; reading resets it), "motion_active" (handles of
 * univst_unet_create_animatediff: the number of motion modules finalize found with a non-zero proj_out) and the name of every option above (its
 * current value; "motion_fold" on the handles that have it). */
int univst_unet_query(univst_unet* h, const char* name, double* out);

/* ------------------------------------------------------------------ temporal VAE handle
 * The VAE behind the pipeline's decode / encode call sites (stable_diffusion.py:369-394 decode_latents, :793-818 get_images_from_latents,
 * :820-834 get_latent_image, ddim_inversion.py:28-31,52-55): diffusers' AutoencoderKLTemporalDecoder (the SVD VAE the reference's run_*_sd.py
 * load, src/sd/run_video_style_transfer_sd.py:36) as one graph of the library's kernels per call.  THIRD-PARTY network, restated from its published
 * definition with that class's state-dict keys (csrc/vae.hip); parity unpinned by the reference. */
typedef struct univst_vae univst_vae;
typedef struct {
    int in_channels, out_channels, latent_channels;      /* 3, 3, 4 */
    int block_out_channels[4];                           /* SVD: 128, 256, 512, 512 (multiples of norm_num_groups and of 8) */
    int layers_per_block;                                /* 2 */
    int norm_num_groups;                                 /* 32 */
} univst_vae_cfg;
int univst_vae_create(const univst_vae_cfg* cfg, univst_vae** out);
int univst_vae_destroy(univst_vae* h);
/* key = diffusers state-dict name ("decoder.up_blocks.0.resnets.1.temporal_res_block.conv1.weight", "quant_conv.bias", ...) */
int univst_vae_load_tensor(univst_vae* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int univst_vae_finalize(univst_vae* h, void* stream);
/* AutoencoderKLTemporalDecoder.decode(z, num_frames).sample: z [imgs, latent, h, w] (imgs = clips x num_frames, already divided by the scaling
 * factor) -> out [imgs, out_channels, 8h, 8w]; the temporal layers couple the num_frames frames of a clip */
int univst_vae_decode(univst_vae* h, const void* z, int64_t imgs, int num_frames, int lat_h, int lat_w, void* out, void* stream);
/* AutoencoderKLTemporalDecoder.encode(x).latent_dist.parameters: x [imgs, in_channels, H, W] in [-1, 1] -> moments [imgs, 2*latent, H/8, W/8]
 * (mean | logvar; sampling stays with the caller, which owns the RNG) */
int univst_vae_encode(univst_vae* h, const void* x, int64_t imgs, int H, int W, void* moments, void* stream);

/* ------------------------------------------------------------------ plain AutoencoderKL handle (the `vae` of the SD3 / SD3.5 pipeline)
 * diffusers' AutoencoderKL (DownEncoderBlock2D / UpDecoderBlock2D x 4, mid_block_add_attention) behind `pipeline.vae.decode / encode`
 * (custom_pipeline.py decode path, inversion_tools/flow_inversion.py latent encoding; src/sd3/run_*_sd3.py load it from `<model>/vae`): the SD3 16-channel
 * VAE, SD-v1.5's image VAE.  The layers of the temporal VAE without the temporal ones, on the same kernels.  THIRD-PARTY network, restated from its
 * published definition with that class's state-dict names (csrc/vae.hip); tests/klvae_ref.py is the yardstick; parity unpinned.  All GroupNorm eps 1e-6.
 *   attn_score_bytes (0: 128 MiB): bound on the fp16 score matrix of the one-head mid-block attention.  The query rows of a frame run in chunks of Qc rows
 *       against all N = H/8 * W/8 keys, Qc the largest multiple of 128 (the GEMM row tile) with Qc * N * 2 <= attn_score_bytes, at least 128, at most N.
 *   pass_bytes (0: 8 GiB): bound on the activation arena.  No layer couples images, so a call runs its batch in groups of the most images whose arena
 *       need stays under it (at least one image; the last group may be smaller); the arena is sized from the group. */
typedef struct univst_klvae univst_klvae;
typedef struct {
    int in_channels, out_channels, latent_channels;      /* 3, 3, 16 (SD3) / 4 (SD-v1.5); latent_channels a multiple of 4 */
    int block_out_channels[4];                           /* 128, 256, 512, 512 (multiples of 8 and even multiples of norm_num_groups) */
    int layers_per_block;                                /* 2 */
    int norm_num_groups;                                 /* 32 */
    int use_quant_conv, use_post_quant_conv;             /* SD3: 0, 0; SD-v1.5: 1, 1 */
    int64_t attn_score_bytes, pass_bytes;
} univst_klvae_cfg;
int univst_klvae_create(const univst_klvae_cfg* cfg, univst_klvae** out);
int univst_klvae_destroy(univst_klvae* h);
/* key = diffusers state-dict name ("decoder.up_blocks.0.resnets.1.conv1.weight", "decoder.mid_block.attentions.0.to_q.weight", ...); the attention
 * weights are [C, C] linears (univst_amd.vae.kl_tensors maps the query / key / value / proj_attn names and 1x1-conv shapes of old checkpoints) */
int univst_klvae_load_tensor(univst_klvae* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
int univst_klvae_finalize(univst_klvae* h, void* stream);
/* AutoencoderKL.decode(z).sample: z [imgs, latent, h, w] (already z / scaling_factor + shift_factor) -> out [imgs, out_channels, 8h, 8w]; h * w a multiple of 8 */
int univst_klvae_decode(univst_klvae* h, const void* z, int64_t imgs, int lat_h, int lat_w, void* out, void* stream);
/* AutoencoderKL.encode(x).latent_dist.parameters: x [imgs, in_channels, H, W] in [-1, 1] -> moments [imgs, 2*latent, H/8, W/8] (mean | logvar; the caller
 * samples).  H, W multiples of 8, H/8 * W/8 a multiple of 8 */
int univst_klvae_encode(univst_klvae* h, const void* x, int64_t imgs, int H, int W, void* moments, void* stream);
/* read-outs of a handle: the shared names of univst_unet_query ("arena_bytes" = the need of the largest group so far: the supported way to size
 * pass_bytes — run a group of g images once, read it, and give it as pass_bytes to get groups of g at that image size), "attn_chunks" (chunks per
 * frame of the attention in the last call), "passes" (groups the last call ran its batch in) */
int univst_klvae_query(univst_klvae* h, const char* name, double* out);

/* ------------------------------------------------------------------ RAFT-large optical flow handle (the `flow_fn` of src/cal_optica_flow.py)
 * The flow estimator behind get_warp (cal_optica_flow.py:51-99) and the sliding-window smoother (stable_diffusion.py:731-747): torchvision's
 * raft_large as one graph of gfx950 kernels per image pair (12 flow updates, final flow only, eval mode).  THIRD-PARTY network, restated from its
 * published definition with that model's state-dict keys (csrc/raft.hip); parity unpinned by the reference. */
typedef struct univst_raft univst_raft;
int univst_raft_create(univst_raft** out);
int univst_raft_destroy(univst_raft* h);
/* key = torchvision state-dict name ("feature_encoder.layer2.0.downsample.0.weight", "update_block.flow_head.conv2.bias", ...); kept in fp32
 * (the BatchNorm fold of the context encoder is done in fp32); the derived fp16 layouts are built by the first call that needs them */
int univst_raft_load_tensor(univst_raft* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
/* img1, img2: uint8 [H, W, 3] (scaled by 1/255 inside: preprocess_image, cal_optica_flow.py:11-13) -> flow fp32 [H, W, 2] (x, y) from img1 to img2.
 * H, W multiples of 8, at least 128.  The workspace is allocated by the first call at a size; later calls at that size neither allocate nor sync. */
int univst_raft_forward(univst_raft* h, const uint8_t* img1, const uint8_t* img2, int H, int W, float* flow, void* stream);
/* stages of the same graph (tests, tools/bench_flow.py).  encode: both encoders -> fmap fp16 [2, N, 256] (image 1 | image 2; N = (H/8)(W/8) rows in
 * y-major order), hidden fp32 [N, 128] = tanh half and context fp16 [N, 128] = relu half of the context encoder (outputs may be NULL).
 * gru: one RecurrentBlock step (convgru1 1x5, convgru2 5x1) over [hidden | context | motion]: hidden fp32 [N, 128] in place, context / motion fp16 [N, 128]. */
int univst_raft_encode(univst_raft* h, const uint8_t* img1, const uint8_t* img2, int H, int W, void* fmap, float* hidden, void* context, void* stream);
int univst_raft_gru(univst_raft* h, float* hidden, const void* context, const void* motion, int fh, int fw, void* stream);
/* corr[i][j] = <fmap1[i], fmap2[j]> / 16 (fmaps fp16 [N, 256]) and its 2x2-average-pooled levels (floor), fp32, level l at
 * [N][fh >> l][fw >> l] behind the levels before it: univst_raft_pyramid_floats(fh, fw) floats in all */
int64_t univst_raft_pyramid_floats(int fh, int fw);
int univst_raft_corr_pyramid(const void* fmap1, const void* fmap2, int fh, int fw, float* pyramid, void* stream);
/* radius-4 lookup at coords fp32 [N, 2] (x, y): channel l*81 + a*9 + b = level l sampled bilinearly (zeros outside) at x / 2^l + (a - 4),
 * y / 2^l + (b - 4).  out_f32 [N, 324] and / or out_f16 [N, 328] (the row the 1x1 conv behind it reads; 4 zero columns) */
int univst_raft_corr_lookup(const float* pyramid, const float* coords, int fh, int fw, float* out_f32, void* out_f16, void* stream);
/* flow fp32 [fh, fw, 2], mask fp16 [N, 576] (the mask predictor's conv output BEFORE its factor 0.25; channel k*64 + i*8 + j) -> out fp32
 * [8 fh, 8 fw, 2]: softmax over the 9 taps k of each sub-pixel (i, j) applied to the 3x3 neighbourhood (zero padded) of 8 * flow */
int univst_raft_convex_upsample(const float* flow, const void* mask, int fh, int fw, float* out, void* stream);

/* ------------------------------------------------------------------ CLIP text tower handle (the `text_encoder` of both pipelines)
 * transformers' CLIPTextModel / CLIPTextModelWithProjection behind `pipeline.text_encoder(ids)` (stable_diffusion.py _encode_prompt,
 * ddim_inversion.py, custom_pipeline.py _get_clip_prompt_embeds) as one graph of gfx950 kernels per call: SD-v1.5's CLIP-L, SD-v2.1's OpenCLIP-H,
 * SD3's CLIP-L and CLIP-bigG.  THIRD-PARTY network, restated from its published definition with that class's state-dict keys (csrc/clip.hip);
 * tests/clip_ref.py is the yardstick and tests/test_clip_ref.py holds it to transformers. */
typedef struct univst_clip univst_clip;
typedef struct {
    int vocab_size;                 /* 49408 */
    int hidden_size;                /* 768 / 1024 / 1280: num_heads * 64 */
    int intermediate_size;          /* 4 * hidden_size */
    int num_layers;                 /* 12 / 23 / 32 */
    int num_heads;                  /* hidden_size / 64 */
    int max_positions;              /* 77 (<= 80) */
    int hidden_act;                 /* 0: quick_gelu  x sigmoid(1.702 x);  1: gelu (exact, erf) */
    float layer_norm_eps;           /* 1e-5 */
    int projection_dim;             /* 0: no text_projection (CLIPTextModel) */
    int eos_token_id;               /* 2: legacy pooling (the position of the largest id); else the first position holding this id, 0 if none */
} univst_clip_cfg;
/* refuses (before any launch) a head dim other than 64 and max_positions beyond 80 */
int univst_clip_create(const univst_clip_cfg* cfg, univst_clip** out);
int univst_clip_destroy(univst_clip* h);
/* key = transformers state-dict name with or without one leading "text_model." ("text_model.encoder.layers.3.mlp.fc1.weight",
 * "embeddings.token_embedding.weight", "text_projection.weight"); dtype 0 = fp16, 1 = fp32 */
int univst_clip_load_tensor(univst_clip* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
/* checks every tensor the config calls for and derives the fused q|k|v weights (the attention scale 1/8 folded into the q rows) */
int univst_clip_finalize(univst_clip* h, void* stream);
/* ids int64 [B, S] (S <= max_positions; an id outside [0, vocab) is clamped) -> any of: last_hidden fp16 [B, S, C] (after final_layer_norm),
 * hidden_states fp16 [L + 1, B, S, C] (the residual streams before final_layer_norm: embeddings, then every layer's output), pooled fp16
 * [B, projection_dim or C] (text_embeds / pooler_output); NULL skips an output.  The first call at a (B, S) sizes the arena; later calls at that
 * size neither allocate nor synchronise. */
int univst_clip_encode(univst_clip* h, const int64_t* ids, int B, int S, void* last_hidden, void* hidden_states, void* pooled, void* stream);
/* read-outs of a handle: the shared names of univst_unet_query, "splitk_bytes" (the split-K workspace the arena holds for the linears of the last (B, S)) */
int univst_clip_query(univst_clip* h, const char* name, double* out);
/* the tower's attention on its own (tests): qkv fp16 [B * S, 3 * heads * 64] = q | k | v rows, q already scaled by 1/8; causal softmax over
 * the S <= 80 positions of each (batch, head) -> out fp16 [B * S, heads * 64] */
int univst_clip_attention(const void* qkv, int B, int S, int heads, void* out, void* stream);

/* ------------------------------------------------------------------ T5 encoder handle (the `text_encoder_3` of the SD3 / SD3.5 pipeline)
 * transformers' T5EncoderModel (encoder stack only, v1.1 gated-gelu form: T5 v1.1-XXL) behind `pipeline.text_encoder_3(ids)[0]`
 * (custom_pipeline.py encode_prompt) as one graph of gfx950 kernels per call.  THIRD-PARTY network, restated from its published definition with
 * that class's state-dict keys (csrc/t5.hip); tests/t5_ref.py is the yardstick and tests/test_t5_ref.py holds it to transformers.  The residual
 * stream is fp32 (T5's outgrows the fp16 range); norms write fp16, linears run fp16 with fp32 accumulation. */
typedef struct univst_t5 univst_t5;
typedef struct {
    int vocab_size;                 /* 32128 */
    int d_model;                    /* 4096 (a multiple of 8) */
    int d_ff;                       /* 10240 (a multiple of 8); feed_forward_proj = "gated-gelu": wi_0 (gelu_new) * wi_1, then wo */
    int num_layers;                 /* 24 */
    int num_heads;                  /* 64; num_heads * d_kv may differ from d_model */
    int d_kv;                       /* 64: the only head dim the attention kernel has */
    int num_buckets;                /* 32: relative_attention_num_buckets */
    int max_distance;               /* 128: relative_attention_max_distance */
    float layer_norm_eps;           /* 1e-6 */
} univst_t5_cfg;
/* refuses (before any launch, naming the field) d_kv other than 64, widths that are no multiple of 8, fewer than 4 buckets */
int univst_t5_create(const univst_t5_cfg* cfg, univst_t5** out);
int univst_t5_destroy(univst_t5* h);
/* key = transformers state-dict name ("encoder.block.3.layer.1.DenseReluDense.wi_0.weight", "encoder.final_layer_norm.weight",
 * "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"); the tied embedding loads as "shared.weight" or
 * "encoder.embed_tokens.weight" (either or both: one copy is kept); dtype 0 = fp16, 1 = fp32 */
int univst_t5_load_tensor(univst_t5* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
/* checks every tensor the config calls for and derives the fused q|k|v and wi_0|wi_1 weights and the per-head bias table [heads][delta + 511] */
int univst_t5_finalize(univst_t5* h, void* stream);
/* ids int64 [B, S] (1 <= S <= 512; an id outside [0, vocab) is clamped) -> last_hidden fp16 [B, S, d_model] (after final_layer_norm).  The first
 * call at a (B, S) sizes the arena; later calls at that size neither allocate nor synchronise. */
int univst_t5_encode(univst_t5* h, const int64_t* ids, int B, int S, void* last_hidden, void* stream);
/* read-outs of a handle: the shared names of univst_unet_query ("weight_bytes" counts the fused copies and the bias table), "splitk_bytes" (the
 * split-K workspace the arena holds for the linears of the last (B, S)) */
int univst_t5_query(univst_t5* h, const char* name, double* out);
/* the encoder's attention on its own (tests): qkv fp16 [B * S, 3 * heads * 64] = q | k | v rows (no scaling is applied), bias_table fp32
 * [heads][1023] indexed by (key position - query position) + 511; bidirectional softmax over the S <= 512 positions of each (batch, head)
 * -> out fp16 [B * S, heads * 64] */
int univst_t5_attention(const void* qkv, const float* bias_table, int B, int S, int heads, void* out, void* stream);
/* host only (no GPU): transformers' T5Attention._relative_position_bucket (bidirectional) for the deltas -(n-1) .. n-1 -> out[2n - 1] */
int univst_debug_t5_buckets(int num_buckets, int max_distance, int n, int* out);

/* ------------------------------------------------------------------ AnimateDiff motion-module handle (the `motion_module` behind every spatial transformer)
 * AnimateDiff-v2's VanillaTemporalModule (backbones/animatediff/models/motion_module.py: per-frame GroupNorm, proj_in, TemporalTransformerBlocks of
 * Temporal_Self attentions along the FRAME axis and a GEGLU feed-forward, proj_out, + input) as one graph of gfx950 kernels per call, on the
 * library's own activation order: row (b * F + f) * N + n, frame-major NHWC (csrc/motion.hip).  Its Attention / FeedForward layers are diffusers'
 * (third-party, restated from their published definition); tests/motion_ref.py is the yardstick and tests/test_motion_ref.py holds it to golden g20. */
typedef struct univst_motion univst_motion;
typedef struct {
    int channels;                   /* 320 / 640 / 1280: num_heads * 40, 80 or 160 */
    int num_heads;                  /* 8 */
    int num_blocks;                 /* num_transformer_block: 1 */
    int attn_per_block;             /* len(attention_block_types), all "Temporal_Self": 2 */
    int norm_groups;                /* 32 */
    int max_len;                    /* temporal_position_encoding_max_len: 24 / 32 (<= 32); the most frames a forward takes */
    int position_encoding;          /* 1: the sinusoid table is added to the input of to_q / to_k / to_v */
    float gn_eps;                   /* 1e-6 */
    float ln_eps;                   /* 1e-5 */
} univst_motion_cfg;
/* refuses (before any GPU call, naming the field) a channels / num_heads other than 40, 80 or 160, channels that are no multiple of norm_groups,
 * max_len outside 1..32 */
int univst_motion_create(const univst_motion_cfg* cfg, univst_motion** out);
int univst_motion_destroy(univst_motion* h);
/* key = the module's state-dict name ("temporal_transformer.proj_in.weight", "temporal_transformer.transformer_blocks.0.attention_blocks.1.to_q.weight",
 * "temporal_transformer.transformer_blocks.0.ff.net.0.proj.bias"); a checkpoint's "...attention_blocks.i.pos_encoder.pe" [1, max_len, channels]
 * replaces the table computed from the formula; dtype 0 = fp16, 1 = fp32 */
int univst_motion_load_tensor(univst_motion* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, void* stream);
/* checks every tensor the config calls for and derives the fused q|k|v weights (the score scale folded into the q rows), the GEGLU projection in
 * the row order of univst_linear's geglu = 1, and per attention the projected position rows pe_qkv[f] = Wqkv pe[f] (fp32 accumulation, fp16 rows) */
int univst_motion_finalize(univst_motion* h, void* stream);
/* X, Y fp16 [B * F, N, channels] rows (Y may not alias X, both 16-byte aligned); F <= 32, and F <= max_len when position_encoding is on.  The first call at a (B, F, N) sizes the arena; later calls at that size
 * neither allocate nor synchronise. */
int univst_motion_forward(univst_motion* h, const void* X, void* Y, int B, int F, int N, void* stream);
/* read-outs of a handle: the shared names of univst_unet_query */
int univst_motion_query(univst_motion* h, const char* name, double* out);
/* the module's attention on its own: softmax attention along the frame axis.  qkv fp16 rows q | k | v, 3 * heads * head_dim wide and ldx halfs apart,
 * row (b * F + f) * N + n, q already carrying the score scale; pe_qkv NULL or fp16 [F][3 * heads * head_dim], row f added to every row of frame f as
 * it is loaded (the sum rounded to fp16 once); bidirectional softmax over the F rows {(b, f', n)} of each (b, n, head) -> out fp16 rows in the same
 * order, heads * head_dim wide and ldo apart.  The rows are read in place (no regrouped copy).  1 <= F <= 32, head_dim 40 / 80 / 160, ldx a
 * multiple of 8 and ldo of 4, B * F * N < 2^31, N * heads <= 2^24, B <= 65535; anything else is UNIVST_ERR_ARG before any launch. */
int univst_temporal_attention(const void* qkv, int64_t ldx, const void* pe_qkv, int B, int F, int N, int heads, int head_dim, void* out, int64_t ldo,
                              void* stream);

/* ------------------------------------------------------------------ AnimateDiff UNet3D: a univst_unet of another kind
 * backbones/animatediff/models/unet.py as animatediff-v2.yaml configures it: the SD-v1.5 2-D UNet run per frame (InflatedConv3d, per-frame
 * InflatedGroupNorm, attn1 with ONE key source — the frame itself —, no attn_temp, no temporal convs) with a motion module (above) behind every
 * resnet / transformer pair: layers_per_block per down block, layers_per_block + 1 per up block, one in the mid block between its transformer and its
 * second resnet (unet_blocks.py:271-276, :382-421, :621-667).  The result is a univst_unet: load_tensor / finalize / reserve / forward / set_option /
 * query / destroy serve it.  State-dict names are the reference's ("down_blocks.i.resnets.j.*", "...attentions.j.transformer_blocks.0.*",
 * "down_blocks.i.motion_modules.j.temporal_transformer.*", "up_blocks.i.motion_modules.j.*", "mid_block.motion_modules.0.*", "conv_norm_out.*",
 * "...pos_encoder.pe").
 *   create   refuses (no GPU call, naming the field) a level width with width / motion.num_heads outside {40, 80, 160} or no multiple of
 *            motion.norm_groups, for every level that has motion modules.
 *   finalize finds on the device the modules whose proj_out (weight and bias) is still all zeros (zero_initialize: no motion checkpoint loaded):
 *            they are skipped EXACTLY, so a UNet with 2-D weights only equals the per-frame 2-D UNet.  A module none of whose tensors was loaded
 *            counts as such a module.
 *   forward  refuses F > 32, F > motion.max_len with position encoding on, and a non-NULL feat_out (the feature tap of this UNet is on univst_unet_forward_tap).
 *            PnP: the same 8 decoder attn1 layers and the same univst_pnp; the window is pnp_utils.py:45 of this backbone,
 *            eta1 * 50 <= idx < eta2 * 50 (exclusive at the top, eta1 scaled); outside it the registered forward equals the stock one bit for bit;
 *            alpha / gamma come from the caller (the reference has 0.8 and 2.0).
 *   univst_unet_set_comm / univst_unet_set_comm_native return UNIVST_ERR_UNSUPPORTED: the frame-axis attention needs every frame on one rank.
 * The motion chain runs on the UNet's arena and split-K workspace (no per-module arena); univst_unet_query("arena_high_water") reports the mark.
 * Option "motion_fold" (univst_unet_set_option): 0 = the chain as univst_motion_forward runs it (default).  1 (GroupNorm statistics from the producer's
 * epilogue folded into proj_in, LayerNorms folded into q|k|v and the GEGLU projection) is NOT BUILT: the value is refused with UNIVST_ERR_UNSUPPORTED. */
typedef struct {
    int inflated_groupnorm;      /* 1: resnet / output GroupNorms per frame (resnet.py:21-29); 0: over all frames (the 5-D route of the SD graph) */
    int motion_levels_mask;      /* bit l: level l has motion modules (motion_module_resolutions [1,2,4,8] -> 15); 0 = use_motion_module false */
    int motion_mid_block;        /* 1: mid_block.motion_modules.0 exists */
    univst_motion_cfg motion;    /* channels is ignored (taken per level); the rest as univst_motion_create checks it, per level's width */
} univst_animatediff_cfg;
int univst_unet_create_animatediff(const univst_unet_cfg* cfg, const univst_animatediff_cfg* ad, univst_unet** out);

/* ------------------------------------------------------------------ stand-alone operators (also used by tests) */
/* Y[M,N] = X[M,K] W[N,K]^T + bias + residual; geglu != 0: the diffusers GEGLU projection (FeedForward net[0], attention.py:241) — writes the
 * N/2 columns x * gelu(gate), W / bias rows pre-interleaved: geglu = 1 in blocks of [16 x rows | 16 gate rows] (any K), geglu = 2 in the
 * order of the X-resident kernel for K = 320 (N % 256 == 0, no residual; univst_geglu_xres_permute makes it from the [x | gate] weight).
 * Replaces torch Linear / 1x1 conv call sites attention.py:123,141,375-377,425.
 * Shapes: M, N >= 1; K % 8 == 0 and ldx % 8 == 0 with X and W 16-byte aligned (the operand tiles move in 16-byte pieces); every other requirement is of
 * the fast paths only.  N, ldy and ldr are otherwise free: rows of Y / residual that are 16-byte aligned (ldy % 8 == 0, ldr % 8 == 0, aligned pointers)
 * take the row-contiguous epilogue of the 256x320 tile, anything else its register epilogue or the 128-wide tile, which store 4 channels (8 bytes) per lane
 * at whatever alignment the row has — with N % 4 != 0 or an odd ldy that is a 2-byte aligned address, which gfx950 global memory accesses allow (slower,
 * not wrong) — and finish a row whose N is not a multiple of 4 element by element.  bias needs 8-byte alignment.  geglu = 1 needs N % 32 == 0. */
int univst_linear(const void* X, int64_t ldx, const void* W, const void* bias, const void* residual, int64_t ldr,
                  void* Y, int64_t ldy, int M, int N, int K, int geglu, void* stream);
/* univst_linear with the rest of the plain epilogue and a caller-held split-K workspace (what the UNet graph passes to the same launcher):
 *   Y = fp16( fp16( X W^T + bias + rowbias[m / rows_per_rowbias] + residual ) + bias2 )
 * rowbias (may be NULL): rows of N halfs, ldrb apart (0: N), one per rows_per_rowbias output rows (the time-embedding add per branch); bias2 (may be
 * NULL): [N], added AFTER the fp16 rounding, so the sum is rounded a second time.  workspace (may be NULL): workspace_bytes of device memory for the fp32
 * partials of a split-K launch, 16-byte aligned; a launch that needs more than it holds (splits * M * N * 4 bytes, see univst_debug_gemm_plan) takes
 * stream-ordered scratch of its own, as it does without one, and computes the same. */
int univst_linear_epi(const void* X, int64_t ldx, const void* W, const void* bias, const void* residual, int64_t ldr, void* Y, int64_t ldy,
                      int M, int N, int K, int geglu, const void* rowbias, int rows_per_rowbias, int64_t ldrb, const void* bias2,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* Row permutation of a GEGLU projection's weight [rows][cols] (or bias / per-row fp16 vector: cols = 1) from the checkpoint's
 * [x rows | gate rows] order into the geglu = 2 order: row nt*256 + wn*64 + i*16 + g*4 + r <- x row (r < 2) or gate row (r >= 2) of hidden
 * column nt*128 + wn*32 + i*8 + g*2 + (r & 1).  rows % 256 == 0. */
int univst_geglu_xres_permute(const void* in, void* out, int rows, int cols, void* stream);
/* The linear with the MM-DiT epilogues of the SD3 path (diffusers JointTransformerBlock / FeedForward, third-party):
 *   Y = residual + gate[m / rows_per_gate] (.) act(X W^T + bias)
 * act: UNIVST_ACT_NONE or UNIVST_ACT_GELU_TANH (defined below); gate (may be NULL): rows of N halfs, ld_gate apart, 16-byte aligned
 * (a chunk of the adaLN linear's [B, 6C] output: rows_per_gate = tokens per frame); residual may be NULL. */
int univst_linear_gated(const void* X, int64_t ldx, const void* W, const void* bias, const void* residual, int64_t ldr, void* Y, int64_t ldy,
                        int M, int N, int K, int act, const void* gate, int64_t ld_gate, int rows_per_gate, void* stream);
/* The same linear with a LayerNorm folded into it and / or row statistics emitted for the next one (what the UNet graph does with
 * norm1/2/3 of a transformer block, attention.py:311-329).  For problems the direct 256x320 tile takes (N % 320 == 0, at least
 * 150 tiles) and, without GEGLU, for problems the 128-wide tile runs without split-K (N % 160 == 0 for stats_out); else
 * UNIVST_ERR_ARG — a split-K problem has its epilogue in the reduction kernel.
 *   stats_out (may be NULL): fp32 [M][N/160][2] <- (sum, sum of squares) of the stored fp16 outputs per 160-column slot.
 *   ln_stats  (may be NULL): fp32 [M][K/160][2] written by the linear that produced X.  Then X holds the RAW rows, W must be
 *             fp16(gamma[k] * W[n][k]), ln_wsum[n] = sum_k of that, ln_bias[n] = bias[n] + sum_k beta[k] W[n][k] (fp32), bias NULL,
 *             and Y = rstd * (X W^T - mean * ln_wsum) + ln_bias  ==  LayerNorm(X) W_orig^T + bias  (+ residual, GEGLU as usual). */
int univst_linear_ln(const void* X, int64_t ldx, const void* W, const void* bias, const void* residual, int64_t ldr,
                     void* Y, int64_t ldy, int M, int N, int K, int geglu, const float* ln_stats, float ln_eps,
                     const float* ln_wsum, const float* ln_bias, float* stats_out, void* stream);
/* The text cross-attention of a transformer block as ONE launch (attention.py:321-327: norm2 -> attn2 -> + hidden_states; the attention itself
 * is diffusers' Attention with 77 text keys, third-party):
 *     Y = to_out( softmax( (LN(X) Wq^T)(text Wk^T)^T / sqrt(d) ) (text Wv^T) ) + bias_o + residual
 * replacing univst_linear_ln (q) + univst_attention (one 77-key source) + univst_linear (out + residual) and the HBM round trips of Q and O.
 *   X [M, ldx] input rows; with ln_stats (fp32 [M][C/160][2], written by the linear that produced X: univst_linear_ln's stats_out) X holds the
 *       RAW rows and Wq_frag is made from fp16(gamma[k] * Wq[n][k]), ln_wsum / ln_bias as in univst_linear_ln; else X is already normalised.
 *   Wq_frag, Wo_frag: the [C, C] weights in MFMA operand order (univst_frag_pack); q_prescaled != 0: Wq already carries log2(e)/sqrt(d).
 *   kv [B*T, 2C]: K | V rows of the text tokens of every branch (T <= 80 keys); rows [b*rows_per_branch, (b+1)*rows_per_branch) of X attend to branch b.
 *   stats_out (may be NULL): fp32 [M][C/160][2] row statistics of Y for a following folded LayerNorm.
 *   workspace: univst_attn2_fused_workspace_bytes(B, heads, head_dim) (K / V of every (branch, head) in operand order).
 * Served: C = 320 with 8 heads (the 64x64 level of SD-v1.x), rows_per_branch % 64 == 0; else UNIVST_ERR_ARG. */
int64_t univst_attn2_fused_workspace_bytes(int B, int heads, int head_dim);
int univst_attn2_fused(const void* X, int64_t ldx, const float* ln_stats, float ln_eps, const float* ln_wsum, const float* ln_bias,
                       const void* Wq_frag, int q_prescaled, const void* kv, int B, int T, int64_t rows_per_branch, const void* Wo_frag,
                       const void* bias_o, const void* residual, int64_t ldr, void* Y, int64_t ldy, int64_t M, int C, int heads,
                       float* stats_out, void* workspace, void* stream);
/* The same with the SELF-attention's out projection in front (attention.py:316-327: attn1.to_out + hidden_states -> norm2 -> attn2 -> + hidden_states):
 *     H2 = attn_out Wp^T + bias_p + residual_in;   Y = to_out( attention( LN(H2) Wq^T, text K, text V ) ) + bias_o + H2
 * H2 — which only this block reads — stays in LDS; its LayerNorm statistics are taken inside (ln_wsum / ln_bias as in univst_linear_ln, Wq_frag from the
 * gamma-folded weight).  Replaces univst_linear_ln (attn1.to_out, stats_out) + univst_attn2_fused.  Same shapes as univst_attn2_fused. */
int univst_attn12_fused(const void* attn_out, int64_t ldx, const void* Wp_frag, const void* bias_p, const void* residual_in, int64_t ldr_in, float ln_eps,
                        const float* ln_wsum, const float* ln_bias, const void* Wq_frag, int q_prescaled, const void* kv, int B, int T,
                        int64_t rows_per_branch, const void* Wo_frag, const void* bias_o, void* Y, int64_t ldy, int64_t M, int C, int heads,
                        float* stats_out, void* workspace, void* stream);
/* W [N][K] (N % 16 == 0, K % 32 == 0) -> the order in which v_mfma_f32_16x16x32_f16 takes it as its A operand: [N/16][K/32][64 lanes][8 halfs],
 * lane (l15, g) = W[nf*16 + l15][ks*32 + g*8 .. +8] — one contiguous 1 KB load per fragment for kernels that read weights straight into registers. */
int univst_frag_pack(const void* W, void* out, int N, int K, void* stream);
/* NHWC implicit-GEMM conv: taps 9 (3x3, pad 1) or 1; optional second source (channel concat), fused nearest x2
 * upsample of the input, stride 1/2.  W is [Cout][taps][C1+C2].  Replaces resnet.py:57-80,145,226. */
int univst_conv_nhwc(const void* X1, const void* X2, int C1, int C2, int imgs, int Hs, int Ws, int upsample, int stride,
                     int taps, const void* W, const void* bias, const void* rowbias, int rows_per_rowbias,
                     const void* residual, void* Y, int Cout, void* stream);
/* the same 3x3 conv with the "tap-inner" weight layout [Cout][(C1+C2)/64][9][64] (C1, C2 multiples of 64): the nine taps
 * of a 64-channel slab are consecutive k tiles, which keeps the re-read activation rows in the XCD's L2. */
int univst_conv_nhwc_tapinner(const void* X1, const void* X2, int C1, int C2, int imgs, int Hs, int Ws, int upsample, int stride,
                              const void* W, const void* bias, const void* rowbias, int rows_per_rowbias,
                              const void* residual, void* Y, int Cout, void* stream);
/* the 3x3 / stride-1 conv (optionally over the nearest x2 upsampled input) from an input patch kept in LDS
 * (conv_patch_kernel): weight layout [Cout][(C1+C2)/32][9][32]
 * (C1, C2 multiples of 32, Cout multiple of 320, image width a multiple of 16, whole image rows per 256/192-row tile, at
 * least 150 tiles — otherwise UNIVST_ERR_ARG: the UNet graph passes both weight copies and falls back by itself).
 * Replaces resnet.py:57-80 for the 64x64 .. 16x16 levels. */
int univst_conv3x3_patch(const void* X1, const void* X2, int C1, int C2, int imgs, int Hs, int Ws, int upsample, const void* W32,
                         const void* bias, const void* rowbias, int rows_per_rowbias, const void* residual, void* Y, int Cout,
                         void* stream);
/* The 3x3 conv over the nearest x2 upsampled input (UpsamplePseudo3D, resnet.py:123-175) as four 2x2-tap PHASE convs over the source image: output pixel
 * (2y+a, 2x+b) sees only 2x2 distinct source pixels, so the weights of phase (a, b) are sums of the original taps (per axis {k0}, {k1+k2} for phase 0 and
 * {k0+k1}, {k2} for phase 1) and the matrix work falls by 9/4.  univst_conv_up2_phase_weights derives the copy W4 [4][Cout][Cin/32][4][32] from the
 * checkpoint's [Cout][Cin][3][3] weight (fp32 sums, one fp16 rounding; Cin % 32 == 0); univst_conv3x3_up2_phase runs conv_patch_kernel in its phase mode
 * on X [imgs][Hs][Ws][C] -> Y [imgs][2Hs][2Ws][Cout] (bias only) and, with gn_out, leaves the GroupNorm statistics of gn_group_width-channel sub-groups
 * per 16-row fragment: gn_out[Cout / width][rows / 16][2] fp32, fragment slot 4 s + phase for source fragment s.  UNIVST_ERR_ARG when the problem is not
 * eligible for the phase form (C % 64, Cout % 320, whole source rows per 256/192-row tile, >= 150 tiles, no split-K): it never falls back silently. */
int univst_conv_up2_phase_weights(const void* W_oihw, int Cout, int Cin, void* W4, void* stream);
int univst_conv3x3_up2_phase(const void* X, int C, int imgs, int Hs, int Ws, const void* W4, const void* bias, void* Y, int Cout, float* gn_out,
                             int gn_group_width, void* stream);
/* Two chained linears with a residual in between, composed into one (the UNet's ff.net.2 -> proj_out, "kcat_fold"):
 *   Wp (W2 m + b2 + tb + r) + bp = [Wp W2 | Wp] [m | r] + (Wp (b2 + tb) + bp)
 * Wp [C][C], W2 [C][K2], b2 / tb / bp [C] fp16 (tb may be null) -> W_out [C][K2 + C] fp16 = [Wp W2 | Wp] and bias_out [C] fp16.  Products and sums are
 * accumulated in fp32 from the fp16 operands and rounded to fp16 once.  C and K2 multiples of 8. */
int univst_linear_compose(const void* Wp, const void* W2, const void* b2, const void* tb, const void* bp, int C, int K2, void* W_out, void* bias_out,
                          void* stream);
/* A GroupNorm folded into the linear that consumes its output (the per-frame GroupNorm -> proj_in of a transformer block, attention.py:121-123): per
 * statistics unit s (rows_per_stat rows) the weight set W_sets[s][n][k] = fp16(W[n][k] * gamma_k * rstd_{s,g(k)}) and the fp32 bias
 * bias32[s][n] = bias[n] + sum_k W[n][k] * (beta_k - mean_{s,g(k)} * rstd * gamma_k); univst_linear_sets then runs on the RAW rows with the set of each
 * row range (rows_per_set = rows_per_stat: a multiple of 256 or 192) — GroupNorm(X) W^T + bias without the normalised copy of X.  stats_out as in
 * univst_linear_ln.  Direct 256x320 problems only (N % 320 == 0, >= 150 tiles); else UNIVST_ERR_ARG. */
int univst_groupnorm_fold_linear(const void* X, int C, int64_t rows, int rows_per_stat, int groups, float eps, const void* gamma, const void* beta,
                                 const void* W, const void* bias, int N, void* W_sets, float* bias32, void* workspace, void* stream);
int univst_linear_sets(const void* X, int64_t ldx, const void* W_sets, const float* bias32, int rows_per_set, const void* residual, int64_t ldr,
                       void* Y, int64_t ldy, int M, int N, int K, float* stats_out, void* stream);
/* GroupNorm(+SiLU) on NHWC rows; rows_per_stat = F*H*W (5-D, stats across frames: resnet.py:338,369) or H*W
 * (per frame: attention.py:121).  workspace: univst_groupnorm_workspace_bytes(). */
int64_t univst_groupnorm_workspace_bytes(int64_t rows, int rows_per_stat, int groups);
int univst_groupnorm_nhwc(const void* X1, const void* X2, int C1, int C2, int64_t rows, int rows_per_stat, int groups,
                          float eps, const void* gamma, const void* beta, int silu, void* Y, void* workspace,
                          void* stream);
/* LayerNorm with affine over the last dim of X [rows, C] (rows in 1 .. INT_MAX; C a multiple of 8 in 8 .. 2048) */
int univst_layernorm(const void* X, void* Y, const void* gamma, const void* beta, int64_t rows, int C, float eps,
                     void* stream);
/* multi-source flash attention.  q rows (bf*Nq+i) at ldq, k/v rows (src*Nkv+j) at ldkv, src_idx int32 [BF][nsrc].
 * Optional (may be NULL): src_cnt int32 [BF] = number of leading sources actually used for that frame, src_logw fp32
 * [BF][nsrc] = log2 multiplicity of a source — a frame that occurs m times in the reference's concatenated key set
 * ([prev, cur, first] at f = 0, 1) is read ONCE with log2(m) added to its scores, which is the same softmax.
 * q_prescaled != 0: q already carries the factor log2(e)/sqrt(head_dim) (the UNet graph folds it into the to_q weights
 * for head_dim 40, so the fastest kernel can take scale and running max inside the QK^T MFMA); 0: plain q.
 * Replaces attention.py:384-420, pnp_utils.py:59-92 and diffusers AttnProcessor2_0. */
int univst_attention(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* out, int64_t ldo,
                     const int32_t* src_idx, const int32_t* src_cnt, const float* src_logw, int nsrc, int BF, int Nq, int Nkv,
                     int heads, int head_dim, int q_prescaled, void* stream);
/* the same attention with the key set of a query split over TWO launches (round 6: a rank of the frame shard consumes the key frames it holds while the
 * halo frames of attention.py:384-413 / pnp_utils.py:59-84 are still on the wire; online softmax does not depend on the order of the keys).
 *   phase 1: state_out != NULL, state_in == NULL — rows of `out` normalised over this launch's sources, state_out[((bf*heads + h)*Nq + i)*2] = (m, l):
 *            the reference of the exponentials in log2 units and the denominator w.r.t. it; a frame with src_cnt[bf] == 0 gets zero rows and l = 0;
 *   phase 2: state_in = phase 1's state_out, `out` = phase 1's rows (read-modify-write): out <- softmax over the UNION of both launches' sources —
 *            exact up to the fp16 rounding of the phase-1 rows; frames with src_cnt[bf] == 0 keep their phase-1 rows.
 * src_cnt is required.  Served at every head_dim of univst_attention. */
int univst_attention_phase(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* out, int64_t ldo,
                           const int32_t* src_idx, const int32_t* src_cnt, const float* src_logw, int nsrc, int BF, int Nq, int Nkv,
                           int heads, int head_dim, int q_prescaled, float* state_out, const float* state_in, void* stream);
/* ---- first vertical slice of the SD3 / SD3.5 rectified-flow path (the reference-owned pieces only) ----
 * The joint-attention processors of backbones/video_diffusion_sd3/pnp_utils.py: CrossFrameProcessor (:17-131; shift = 0) and
 * AttentionShiftProcessor (:143-271; shift = 1 applies the AdaIN shift with alpha 0.8 / gamma 2.0 and the given beta.  The window test
 * eta1*50 <= idx <= eta2*50 and beta = 0.9 -> 0.1 over the window are evaluated by the CALLER in double, as the reference's Python does
 * (pnp_utils.py:183-186) — in fp32, eta1 = 0.3 makes 0.3f*50 = 15.000001 and step 15 falls out of the window — under the documented
 * fixed reading thresh2 == eta2: the reference reads an attribute it never sets).  hidden [B, N, Cin] image tokens of
 * B = (branches x clip_length) frames, enc [B, Nt, Cin] text tokens or NULL; keys of frame f = image tokens of ['first', f-1, f]
 * of its clip (read by pointer) ++ its text tokens (one extra key segment); out_img [B, N, Cin], out_txt [B, Nt, Cin].
 * clip_length == 0: no cross-frame gather — keys of frame f are its own image tokens ++ its text tokens (diffusers' stock
 * JointAttnProcessor2_0, what the MM-DiT runs before register_spatial_attention_pnp / with no processor set).
 * Weights are diffusers' Attention parameters, fp16 device pointers, [out, in] row-major; NULL = absent (biases, the RMS norms of
 * SD3-medium, to_add_out when context_pre_only). */
typedef struct {
    const void *to_q, *to_q_bias, *to_k, *to_k_bias, *to_v, *to_v_bias;             /* [heads*head_dim, Cin] */
    const void *norm_q, *norm_k;                                                    /* [head_dim] RMSNorm weights (SD3.5) */
    const void *add_q, *add_q_bias, *add_k, *add_k_bias, *add_v, *add_v_bias;       /* added (text) projections */
    const void *norm_added_q, *norm_added_k;
    const void *to_out, *to_out_bias, *to_add_out, *to_add_out_bias;                /* [Cin, heads*head_dim] */
} univst_sd3_attn_weights;
/* optional: the MM-DiT block's gated residuals fused into the two out-projections (diffusers JointTransformerBlock:
 * hidden + gate_msa[:, None] * attn_output): out_img = res_img + gate_img[b] (.) to_out(o), out_txt likewise through to_add_out.
 * gate_*: rows of Cin halfs, ld_gate_* apart (chunks of the two adaLN linears' outputs), one per frame b. */
typedef struct {
    const void *res_img, *gate_img, *res_txt, *gate_txt;
    int64_t ld_gate_img, ld_gate_txt;
} univst_sd3_gated_residual;
/* the window test and beta of AttentionShiftProcessor in double (pnp_utils.py:183-186, fixed reading thresh2 == eta2), for callers outside Python:
 * active = eta1*50 <= idx <= eta2*50, beta = 0.9 -> 0.1 over the window (0 outside).  Pass (shift = active, beta) to univst_sd3_joint_attention. */
int univst_sd3_shift_window(int idx, double eta1, double eta2, int* active, float* beta);
int univst_sd3_joint_attention(const univst_sd3_attn_weights* w, const void* hidden, const void* enc, int B, int N, int Nt, int Cin,
                               int heads, int head_dim, int clip_length, int shift, float beta, float rms_eps,
                               void* out_img, void* out_txt, const univst_sd3_gated_residual* gated_residual /* may be NULL */,
                               univst_comm* comm /* may be NULL */, void* stream);
/* comm (frame shard, world > 1): the batch holds frames [rank*clip_length, (rank+1)*clip_length) of every branch; K | V of the clip's
 * first frame (from rank 0) and of the frame before this rank's first one (from rank - 1) arrive through the communicator's peer
 * writes (one exchange + one one-float all-reduce as a barrier per call; workspace >= 64 KiB + 6 x branches*N*Cin fp16: since round 6 a pack is the layer's HIDDEN rows of a boundary frame, posted on the communicator's forked
 * stream at the start of the op; the receiving rank projects them to K | V, applies the k RMSNorm and the shift, and attends in two phases). */
/* ---- MX-fp8 q | k | v projections (BASELINE config 5, "MFMA fp8 QKV"); an option, fp16 stays the default ----
 * Format: OCP MX with e4m3fn elements (OCP, not fnuz): blocks of 32 consecutive K elements, one E8M0 scale byte per block.
 *   block scale  e = floor(log2(amax)) - 8, and e += 1 when amax * 2^-e > 448, amax = max|x| of the block's fp16 values; amax == 0 -> e = 0;
 *                scale byte = e + 127.  With this rule no element saturates.
 *   elements     x * 2^-e (exact) rounded to e4m3 to nearest even.  NaN / Inf inputs are not defined.
 * univst_mxfp8_quantize: X fp16 rows (row stride ldx elements, a multiple of 8; 16-byte aligned) -> Q e4m3 bytes [rows][K], S E8M0 bytes
 * [rows][K/32].  K % 32 == 0. */
int univst_mxfp8_quantize(const void* X, int64_t ldx, int64_t rows, int K, void* Q, void* S, void* stream);
/* Y[M,N] = deq(X) deq(W)^T + bias: Xq [M][K] / Wq [N][K] e4m3 bytes with Xs [M][K/32] / Ws [N][K/32] scale bytes, bias fp16 [N] or NULL,
 * Y fp16 (row stride ldy, a multiple of 4).  Products accumulate in fp32 inside the block-scaled MFMA, the bias is added in fp32, one rounding to
 * fp16 on store.  K % 128 == 0, N % 16 == 0, any M >= 1; anything else is UNIVST_ERR_ARG before any launch. */
int univst_linear_mxfp8(const void* Xq, const void* Xs, const void* Wq, const void* Ws, const void* bias, void* Y, int64_t ldy, int64_t M, int N,
                        int K, void* stream);
/* the quantised FUSED q | k | v weights of one attention module: [3C][Cin] e4m3 bytes and [3C][Cin/32] scale bytes of the consecutive
 * to_q | to_k | to_v (and add_q | add_k | add_v; NULL when the call has no text stream) */
typedef struct {
    const void *qkv, *qkv_scale, *add_qkv, *add_qkv_scale;
} univst_sd3_mx_weights;
/* univst_sd3_joint_attention with the two q | k | v projections in MX-fp8: the op quantises its input rows into its own stream-ordered scratch
 * (rows * Cin * (1 + 1/32) bytes more) and runs univst_linear_mxfp8 against `mx`; biases still come from `w`, and everything behind the
 * projections is the code of univst_sd3_joint_attention.  mx == NULL is univst_sd3_joint_attention itself, launch for launch.
 * With mx: Cin % 128 != 0, or q | k | v weights / biases of `w` that are not consecutive (the fused layout), is UNIVST_ERR_ARG; a communicator
 * of world > 1 is UNIVST_ERR_UNSUPPORTED (the receiver-side projection of the halo rows is not built in MX-fp8). */
int univst_sd3_joint_attention_mx(const univst_sd3_attn_weights* w, const void* hidden, const void* enc, int B, int N, int Nt, int Cin,
                                  int heads, int head_dim, int clip_length, int shift, float beta, float rms_eps,
                                  void* out_img, void* out_txt, const univst_sd3_gated_residual* gated_residual /* may be NULL */,
                                  univst_comm* comm /* may be NULL */, void* stream, const univst_sd3_mx_weights* mx /* may be NULL */);
/* the shift alone, in place on a fused [3*F*N, 3C] q | k | v buffer (branch 0 content, 1 style, 2 stylised; row stride ld):
 * q2 <- gamma*(alpha*q0 + (1-alpha)*q2);  k2 <- beta*AdaIN(k2; k1) + (1-beta)*k1 (same for v) with the SD3 plugin's AdaIN
 * (pnp_utils.py:289-302: F.instance_norm over (N, head_dim) jointly per (frame, head), style mean / unbiased std per channel over N).
 * ws: 4*F*2C + 2*F*2*heads floats. */
int univst_sd3_adain_shift(void* qkv, int64_t ld, int F, int N, int C, int heads, float alpha, float beta, float gamma, void* ws,
                           void* stream);
/* ---- static style branch of the SD3 path (opt-in) ----
 * The style input is ONE image: F identical style frames give every frame the key set [own image keys x 3 ++ own text keys], which is the
 * joint attention at B = 1, clip_length = 1, and the stylised branch reads nothing of the style branch but its post-RMSNorm K | V image rows.
 * So the style runs as one frame whose K | V rows are kept in a caller-owned bank [N, 2C] per attention module, and the other two branches
 * run as a two-branch batch that shifts against the bank.
 *
 * The shift of univst_sd3_adain_shift on a TWO-branch fused buffer qkv2 [2*F*N, 3C] (branch 0 content, 1 stylised; row stride ld), in place on
 * the stylised rows: the style K | V rows come from style_kv [N, 2C] (row stride ld_style >= 2C) and token n of EVERY frame blends against
 * style row n; the style mean / unbiased std per channel over N are taken once, the stylised branch's joint (N, head_dim) statistics per
 * (frame, head) as in the three-branch entry.  Same row arithmetic as the three-branch entry (one device function).  Content rows, style_kv
 * and every column behind 3C / 2C are never written.
 * UNIVST_ERR_ARG before any launch: a null qkv2 / style_kv / ws, N < 2, C % heads != 0, C % 8 != 0, ld % 8 != 0 or ld < 3C, ld_style % 8 != 0 or
 * ld_style < 2C, qkv2 or style_kv not 16-byte aligned (rows move in 16-byte pieces).
 * ws: (2 + 2*F)*2C + 2*F*2*heads floats. */
int univst_sd3_adain_shift_static(void* qkv2, int64_t ld, const void* style_kv, int64_t ld_style, int F, int N, int C, int heads, float alpha,
                                  float beta, float gamma, void* ws, void* stream);
/* univst_sd3_joint_attention_mx (mx may be NULL: fp16 projections) without a communicator, in one of the two roles of the static style branch:
 *   role 0, the bank call: the ordinary joint attention of the style batch (normally B = 1, clip_length = 1: sd3_index_kernel merges the frame's
 *           three identical sources into one of weight log2 3), which also writes frame 0's post-norm K | V image rows [N, 2C] into the
 *           caller-owned style_kv (row stride ld_style).  shift must be 0: the style branch is never shifted.
 *   role 1, the apply call: B = 2 * clip_length, content frames then stylised frames.  With shift != 0 univst_sd3_adain_shift_static runs
 *           against style_kv where the three-branch shift sits (after the q / k RMSNorm, before the cross-frame gather); with shift == 0 style_kv
 *           may be NULL and the call is univst_sd3_joint_attention on the two-branch batch.
 * UNIVST_ERR_ARG before any launch: role not 0 / 1, shift != 0 in role 0, B != 2 * clip_length in role 1, N < 2 in role 1 with shift != 0, a NULL style_kv where the role needs
 * it, ld_style % 8 != 0 or ld_style < 2C, style_kv not 16-byte aligned; everything univst_sd3_joint_attention_mx refuses. */
int univst_sd3_joint_attention_static(const univst_sd3_attn_weights* w, const void* hidden, const void* enc, int B, int N, int Nt, int Cin,
                                      int heads, int head_dim, int clip_length, int shift, float beta, float rms_eps,
                                      void* out_img, void* out_txt, const univst_sd3_gated_residual* gated_residual /* may be NULL */,
                                      void* stream, const univst_sd3_mx_weights* mx /* may be NULL */, void* style_kv, int64_t ld_style, int role);
/* diffusers RMSNorm over the head dim, in place: x[r, h*d + e] *= rsqrt(mean_e x^2 + eps) * weight[e]  (row stride ld >= heads*d) */
int univst_rmsnorm_heads(void* x, int64_t ld, int64_t rows, int heads, int head_dim, const void* weight, float eps, void* stream);
/* the same on two column blocks of one row-strided buffer, as the joint attention runs it on a fused q | k | v row: the heads * head_dim
 * columns at c0 with w0, times scale0 (the softmax scale folded into q), and those at c1 with w1.  The blocks are disjoint and inside ld;
 * every other column is left as it is. */
int univst_rmsnorm_heads_pair(void* x, int64_t ld, int64_t rows, int heads, int head_dim, int64_t c0, const void* w0, int64_t c1,
                              const void* w1, float eps, float scale0, void* stream);
/* y = LayerNorm(x; no affine, eps) * (1 + scale[b]) + shift[b]: AdaLayerNormZero / ZeroX / Continuous of the MM-DiT blocks (diffusers
 * normalization.py, third-party).  x, y [rows, C] (C % 8 == 0, <= 4096); scale / shift are rows of a [rows / rows_per_batch, ...]
 * matrix ld_mod halfs apart (chunks of the adaLN linear's output).  y2 / scale2 / shift2 (all NULL or all set): a second modulation
 * of the same normalised rows (AdaLayerNormZeroX, the dual-attention blocks of SD3.5-medium).  Every pointer of this entry, of
 * univst_gate_residual and of univst_activation is 16-byte aligned (chunk views at multiples of C of a torch allocation are). */
int univst_adaln_modulate(const void* x, void* y, const void* scale, const void* shift, int64_t ld_mod, int64_t rows, int64_t rows_per_batch,
                          int C, float eps, void* y2, const void* scale2, const void* shift2, void* stream);
/* out = x + gate[b] * y: the gated residuals of diffusers' JointTransformerBlock (gate rows ld_gate halfs apart; out may alias x) */
int univst_gate_residual(const void* x, const void* gate, int64_t ld_gate, const void* y, void* out, int64_t rows, int64_t rows_per_batch, int C,
                         void* stream);
/* elementwise activation, fp32 arithmetic (n % 8 == 0; out may alias x): SiLU (adaLN / timestep / pooled-text MLPs) and GELU(tanh)
 * (FeedForward activation_fn="gelu-approximate") */
#define UNIVST_ACT_SILU 0
#define UNIVST_ACT_GELU_TANH 1
#define UNIVST_ACT_NONE (-1)
int univst_activation(const void* x, void* out, int64_t n, int act, void* stream);
/* diffusers Timesteps / get_timestep_embedding: t fp32 [B] (device) -> out fp16 [B, dim] = [sin | cos](t * freq) (halves swapped when
 * flip_sin_to_cos), freq_i = exp(-ln(max_period) i / (dim/2 - downscale_freq_shift)), fp32 arithmetic */
int univst_timestep_embedding(const float* t, void* out, int B, int dim, int flip_sin_to_cos, float downscale_freq_shift, float max_period,
                              void* stream);
/* PatchEmbed's strided conv as a linear: latents [B, C, H, W] -> rows [B*(H/p)*(W/p), C*p*p] in the k order of the flattened conv
 * weight; and the inverse for proj_out's rows [.., p*p*C] ((u, v, c) order) -> latents (transformer_3D_model.py:95-103) */
int univst_sd3_patchify(const void* latents, void* rows, int B, int C, int H, int W, int patch, void* stream);
int univst_sd3_unpatchify(const void* rows, void* latents, int B, int C, int H, int W, int patch, void* stream);
/* out = a*x + b*y + c*z (fp16 storage, fp32 arithmetic): the updates of rf_inversion / rf_solver (flow_inversion.py:123-264) */
int univst_axpbypcz(const void* x, const void* y, const void* z, void* out, float a, float b, float c, int64_t n, void* stream);

/* AdaIN-guided attention shift in place on the fused QKV buffer [3*F*N, 3C]; stats_ws: 4*F*2C floats.
 * Replaces pnp_utils.py:47-57 + attention_adain :114-125. */
int univst_attention_adain_shift(void* qkv, int64_t ld, int F, int N, int C, float alpha, float beta, float gamma,
                                 void* stats_ws, void* stream);
/* The same shift where the style is ONE frame held elsewhere: qkv is the fused buffer of TWO branches [2*F*N, ld >= 3C] (content rows, then stylised
 * rows), style_kv one frame of style K | V rows [N, ld_style >= 2C].  Every frame f reads the same style rows, and one set of column statistics —
 * computed here from style_kv on every call, not precomputed — serves all frames: per element the arithmetic of univst_attention_adain_shift on a
 * three-branch buffer whose style branch is that frame repeated F times.  Only the first 3C columns of the stylised rows are written.  stats_ws: 4C floats.
 * C % 8 != 0, C > 2048, ld or ld_style no multiple of 8, ld < 3C, ld_style < 2C, F or N < 1: UNIVST_ERR_ARG before any launch. */
int univst_attention_adain_shift_static(void* qkv, int64_t ld, const void* style_kv, int64_t ld_style, int F, int N, int C, float alpha, float beta,
                                        float gamma, void* stats_ws, void* stream);
/* latent_adain on [1,C,F,H,W] (pnp_utils.py:128-139) */
int univst_latent_adain(const void* cnt, const void* sty, void* out, int C, int F, int HW, void* stream);
/* the same in two halves for frame shards: stats[c] = {sum, sumsq} of the content over the LOCAL (F,H,W) (the caller
 * all-reduces them), then apply with the global element count n_total = F_total*H*W */
int univst_latent_adain_stats(const void* cnt, float* stats2c, int C, int F, int HW, void* stream);
int univst_latent_adain_apply(const void* cnt, const void* sty, const float* stats2c, int64_t n_total, void* out, int C,
                              int F, int HW, void* stream);
/* out = cx*x + ce*eps: DDIMScheduler.step / next_step with host-folded coefficients (stable_diffusion.py:761,
 * ddim_inversion.py:190-204) */
int univst_axpby(const void* x, const void* eps, void* out, float cx, float ce, int64_t n, void* stream);
/* out = (1-m)*a + m*b, m [F,h,w] broadcast over C (stable_diffusion.py:687-702); m NULL => m = 0 */
int univst_mask_blend(const void* a, const void* b, const void* m, void* out, int C, int64_t FHW, void* stream);
/* uint8 {0,1} mask [F,H,W] -> fp16 [F,h,w], torch bilinear align_corners=False (stable_diffusion.py:689) */
int univst_mask_resize(const uint8_t* mask, void* out, int F, int H, int W, int h, int w, void* stream);

/* ------------------------------------------------------------------ mask propagation (src/mask_propagation.py:72-83,60-69) */
/* one target frame: feat_tar [hw,C] f32, feat_src [Nsrc,C] f32 (row-major, un-normalised), segs_src [ncls,Nsrc] f32
 * -> segs_tar [ncls,hw] f32.  workspace: univst_maskprop_workspace_bytes(). */
int64_t univst_maskprop_workspace_bytes(int hw, int Nsrc, int C);
int univst_maskprop_frame(const float* feat_tar, const float* feat_src, const float* segs_src, float* segs_tar, int hw,
                          int Nsrc, int C, int ncls, float temperature, int topk, void* workspace, void* stream);
/* segs [ncls,h,w] f32 -> bilinear up to [H,W], per-class min-max, first-max argmax, !=0 -> 255 : uint8 [H,W] */
int univst_maskprop_finalize(const float* segs, uint8_t* mask_out, int ncls, int h, int w, int H, int W, void* workspace,
                             void* stream);

/* ------------------------------------------------------------------ flow warp + occlusion + window blend
 * (src/cal_optica_flow.py:20-46, stable_diffusion.py:731-751) */
/* acc[H,W,3] f32 += get_warp(key, now): occlusion ||(c+fwd)+bwd-c|| > thr, cv2.remap-exact bilinear warp of `now`
 * by fwd, occluded pixels take `key`.  key/now uint8 [H,W,3], fwd/bwd f32 [H,W,2]. */
int univst_warp_accumulate(const uint8_t* key, const uint8_t* now, const float* fwd, const float* bwd, float* acc, int H,
                           int W, float threshold, void* stream);
/* The whole window mean of ONE key frame in one launch (stable_diffusion.py:731-747, the inner loop over bias = -r .. r): frames
 * uint8 [F,H,W,3] is the Gauss-Seidel working copy, frame `key` is replaced in place by trunc(mean of {itself, get_warp(key, key+b)});
 * flows: HOST array of 2*nn device pointers, fp32 [H,W,2] each — (forward key -> key+b, backward key+b -> key) of the nn in-clip
 * neighbours in increasing b (r <= 4).  Same arithmetic as univst_warp_accumulate + univst_accumulate_u8 + univst_window_store
 * (bit-identical), 1 launch instead of 2r + 2. */
int univst_warp_window_key(uint8_t* frames, const float* const* flows, int nn, int F, int H, int W, int key, int r, float threshold,
                           void* stream);
/* latent-space sliding window (no reference code exists for it — definition in csrc/warp.hip and DESIGN.md):
 * x0 [C,F,h,w] fp16 in place, lflow [F, 2r+1, h, w, 2] fp32 = flow from frame k to frame k+b in latent-pixel units. */
int univst_latent_window_smooth(void* x0, const float* lflow, int C, int F, int h, int w, int r, float thr, void* stream);
int univst_accumulate_u8(const uint8_t* frame, float* acc, int64_t n, void* stream);
/* dst[i] = (uint8) trunc(acc[i] / weight) */
int univst_window_store(const float* acc, float weight, uint8_t* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------ per-kernel-class HIP-event timing (bench.py roofline leg)
 * classes (one per kernel symbol): 0 gemm_big<0>, 1 gemm_big<1> (conv), 2 gemm_kernel<*,0> (linear), 3 gemm_kernel<*,1>
 * (conv), 4 attention d=40, 5 attention d=80, 6 other attention, 7 groupnorm, 8 layernorm, 9 adain shift, 10 text attention,
 * 11 conv_patch_kernel (LDS-patch 3x3 convs), 12 attn2_fused_kernel, 13 linear_mxfp8_kernel (the MX-fp8 linear; its quantise pass is not bracketed).
 * While enabled every launch of these classes is bracketed by hipEvents on its stream; collect() waits for
 * them and returns per class: summed ms, launch count, algorithmic flops and algorithmic bytes. */
#define UNIVST_PROFILE_CLASSES 14
int univst_profile_enable(int on);
int univst_profile_collect(double* ms, int64_t* count, double* flops, double* bytes, int nclasses);
/* per class, for the records the LAST univst_profile_collect returned: the EXPANDED operand bytes of the GEMM classes — for a 3x3 conv `bytes` above
 * charges input + weights + output (what has to cross HBM once), this figure charges the im2col operand M x 9Cin the matrix pipe consumes */
int univst_profile_collect_aux(double* aux_bytes, int nclasses);
/* ';'-joined kernel symbols launched in class `cls` since profiling was last switched on (template arguments without spaces, e.g.
 * "gemm_big_kernel<0,4,2>"; classes whose launchers do not name their kernels give ""): bench.py quotes PMC traffic only when every one of them
 * has an entry in the committed counter file */
int univst_profile_symbols(int cls, char* buf, int n);

/* bring-up aid: what ds_read_b64_tr_b16 returns per lane for a known LDS image (256 floats) */
int univst_debug_tr16(float* out256, void* stream);
/* measurement aid (bench.py --emulate-wire): a one-thread kernel that keeps `stream` busy for `us` microseconds — the stand-in for a transfer of
 * bytes / link rate when one rank of a multi-GPU job is emulated on a 1-GPU box */
int univst_debug_delay_us(double us, void* stream);

/* What the GEMM / conv launcher and the attention launcher would do for a problem, read out on the host: no GPU, no stream, no device pointers
 * (every kernel-selection decision of the library is made by plain host code; tests/test_dispatch_plan.py holds it to a recorded table).  buf receives
 *     <kernel symbol> grid=<blocks> block=<threads> splits=<s>[ +splitk_reduce]
 * followed, for the GEMM, by the predicates the UNet graph consults for that shape and by what the launcher sets for the 256x320 kernels (the epilogue
 * form: 0 registers, 1 rows through LDS, 3 the GEGLU slab; the tile order in groups of tile_gm row tiles x tile_gn column tiles, 0: column tile fastest):
 *      big_direct=<0|1> fold_producer=<0|1> fold_consumer=<0|1> geglu_consumer=<0|1> geglu_xres=<0|1> epi_lds=<0|1|3> tile_gn=<n> tile_gm=<n>
 * or, with the launcher's non-zero return code, the launcher's error message.  Operands are 16-byte aligned with natural leading dimensions unless a flag
 * says otherwise.  ncu: compute units to plan for (an MI355X has 256).
 * gemm: mode 0 = linear [M, K] x [N, K]^T (geglu as univst_linear; rows_per_set > 0: weight sets with an fp32 bias, as univst_linear_sets);
 *       mode 1 = conv over M images of Hs x Ws with C1 + C2 channels (K is derived), as univst_conv_nhwc, or with one of the VAE's geometries.
 * M = N = 0 (Nq = Nkv = 0): buf receives the ';'-joined kernel symbols the launcher can launch. */
#define UNIVST_PLAN_BIAS 1
#define UNIVST_PLAN_RESIDUAL 2
#define UNIVST_PLAN_ROWBIAS 4
#define UNIVST_PLAN_LN_STATS 8        /* a LayerNorm folded into this linear (univst_linear_ln's ln_stats / ln_wsum / ln_bias) */
#define UNIVST_PLAN_STATS_OUT 16      /* row statistics of the output (univst_linear_ln's stats_out) */
#define UNIVST_PLAN_ACT 32            /* univst_linear_gated: GELU(tanh) */
#define UNIVST_PLAN_GATE 64           /* univst_linear_gated: gate rows */
#define UNIVST_PLAN_W32_ONLY 128      /* only the LDS-patch weight copy (univst_conv3x3_patch) */
#define UNIVST_PLAN_W32 256           /* the LDS-patch weight copy beside the plain one (the UNet graph) */
#define UNIVST_PLAN_GN_OUT 512        /* GroupNorm statistics of 10-channel sub-groups from the epilogue (the UNet graph) */
#define UNIVST_PLAN_TAPINNER 1024     /* univst_conv_nhwc_tapinner's k order */
#define UNIVST_PLAN_Y_UNALIGNED 2048  /* the output is 8 bytes off a 16-byte boundary */
#define UNIVST_PLAN_WORKSPACE 4096    /* the caller holds the split-K workspace (the UNet graph, RAFT) */
#define UNIVST_PLAN_W4 8192           /* the phase weight copy of an upsampler conv beside the others (the UNet graph; univst_conv_up2_phase_weights) */
#define UNIVST_PLAN_LDY_ODD 16384     /* ldy = N + 1: output rows that are not 16-byte aligned */
#define UNIVST_PLAN_GEOM_3X3 0        /* 3x3 with padding 1 (taps = 9) or 1x1 (taps = 1) */
#define UNIVST_PLAN_GEOM_PAD_END 1    /* 3x3 over an input padded at the bottom / right only (the VAE encoder's stride-2 conv) */
#define UNIVST_PLAN_GEOM_FRAME 2      /* 3x1 (taps = 3) over image rows = frames, image columns = pixels (the VAE's Conv3d (3,1,1)) */
int univst_debug_gemm_plan(int ncu, int mode, int M, int N, int K, int geglu, int flags, int rows_per_set, int C1, int C2, int Hs, int Ws, int upsample,
                           int stride, int taps, int geom, char* buf, int n);
#define UNIVST_PLAN_SRC_LOGW 1        /* per-source log2 multiplicities */
#define UNIVST_PLAN_EXTRA_KEYS 2      /* the extra key segment (77 text tokens of the SD3 joint attention) */
/* phase 0: univst_attention; 1 / 2: the first / the merge launch of univst_attention_phase */
int univst_debug_attention_plan(int BF, int heads, int Nq, int Nkv, int nsrc, int d, int q_prescaled, int flags, int phase, char* buf, int n);

/* What univst_groupnorm_nhwc / univst_groupnorm_fold_linear (and the UNet graph's GroupNorms) would launch, read out on the host like the two plans above.
 * has_fold: 0, or the output rows N of the linear the normalisation is folded into; world: ranks the statistics are summed over (1: none);
 * has_producer_stats: every source comes with the statistics its producer's epilogue left.  out_ints receives UNIVST_GN_PLAN_INTS values:
 *   [0] route: 0 small (one launch of gn_small_kernel), 1 streaming (gn_partial_kernel + gn_reduce_chunks_kernel), 2 streaming from producer statistics
 *   [1] fold (the tail is gn_fold_linear_kernel, not gn_apply_kernel)     [2] sharded statistics
 *   [3] block, [4] TR of the streaming kernels: block = (C / 8) * TR threads (0 where none of them runs)
 *   [5] nchunk, [6] rpc: chunks per stat unit and rows per chunk of the statistics pass
 *   [7] nblk, [8] rpb: blocks per stat unit and rows per block of the apply pass
 *   [9], [10] dynamic LDS bytes of the statistics kernel and of the tail
 *   [11], [12] grid of the statistics kernel; [13] grid of the reduction; [14], [15] grid of the tail (0: not launched)
 * or, with a non-zero return code, the launcher's error message is in univst_last_error(). */
#define UNIVST_GN_PLAN_INTS 16
int univst_debug_groupnorm_plan(int C1, int C2, int64_t rows, int rows_per_stat, int G, int has_fold, int world, int has_producer_stats, int* out_ints);

#ifdef __cplusplus
}
#endif
#endif
