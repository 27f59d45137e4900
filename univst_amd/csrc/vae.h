// VAE handle internals (see vae.hip).
#pragma once
#include <string>
#include <unordered_map>

#include "../../include/univst.h"
#include "model.h"

long uv_vae_attn_chunk_rows(long score_bytes, long N);      // query rows per attention chunk under a score budget (vae.hip)

struct Vae : Model {
    univst_vae_cfg cfg;
    std::unordered_map<std::string, float> mix;       // ST-resblock prefix -> time_mixer.mix_factor

    Vae() : Model("vae") {}
    int finalize(hipStream_t s);
    // the arena formula of both handles: `wide` = the widest channel count at the full resolution, score_rows = the query rows of one attention chunk
    size_t arena_need(long imgs, int H, int W, int wide, long score_rows) const;
    int reserve(long imgs, int H, int W);
    int decode(const half_t* z, long imgs, int num_frames, int h, int w, half_t* out, hipStream_t s);
    int encode(const half_t* x, long imgs, int H, int W, half_t* moments, hipStream_t s);
};

// The plain AutoencoderKL (the SD3 / SD3.5 VAE, SD-v1.5's image VAE): the layers of Vae without the temporal ones, on the same store, arena and
// forward helpers.  The base's cfg is filled from kcfg; `mix` stays empty.
struct KlVae : Vae {
    univst_klvae_cfg kcfg;
    long attn_chunks = 0, passes = 0;      // read-outs of the last decode / encode

    long score_bytes() const { return kcfg.attn_score_bytes > 0 ? (long)kcfg.attn_score_bytes : 128L << 20; }
    size_t need_bytes(long imgs, int H, int W) const;      // the arena for a group of imgs images of H x W pixels
    long group_of(long imgs, int H, int W) const;          // images per pass: the most whose need stays under pass_bytes, at least one
    int decode(const half_t* z, long imgs, int h, int w, half_t* out, hipStream_t s);
    int encode(const half_t* x, long imgs, int H, int W, half_t* moments, hipStream_t s);

  private:
    int decode_pass(const half_t* z, long imgs, int h, int w, half_t* out, hipStream_t s);      // one group (an encode pass is VFwd::encoder itself)
};
