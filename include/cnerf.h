/*
 * cnerf.h -- C ABI of libcnerf_hip.so: the MI355X (gfx950) render path of the conditioned-NeRF GAN.
 *
 * The reference has no FFI layer; its boundary for this path is the Python generator API
 *   generators/generators.py:33-187   ImplicitGenerator3d.forward(z, cam2worlds, img_size, fov, ...)
 *   generators/siren.py:637-668       <SIREN variant>.forward(points, z, img_size, num_steps)
 * Each entry point below names the reference code it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer on the current HIP device unless the comment says "host";
 *   - nothing is allocated, freed or synchronised here: the caller passes every buffer, including the
 *     workspace sized by cnerf_workspace_bytes(), and a stream (hipStream_t passed as void*);
 *   - all launches go to that stream; calls are re-entrant, there is no global state;
 *   - return value: 0 on success, a negative CNERF_E* code otherwise; never throws.
 *   - rays: P = R*R per image, pixel p = row*R + col; points per pass N = P*S per image.
 */
#ifndef CNERF_H
#define CNERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNERF_ABI_VERSION 10

#define CNERF_OK 0
#define CNERF_EINVAL (-22)  /* bad argument / unsupported shape (message via cnerf_last_error) */
#define CNERF_ENOSYS (-38)  /* feature not built into this library */
#define CNERF_ELAUNCH (-5)  /* the HIP runtime refused a launch */

#define CNERF_MAX_LAYERS 16
#define CNERF_MAX_LEVELS 4  /* feature-pyramid levels (siren.py:1444-1473) */

/* cnerf_cfg.flags */
#define CNERF_F_HIERARCHICAL (1u << 0) /* generators.py:110  coarse pass + importance resampling + fine pass */
#define CNERF_F_WHITE_BACK (1u << 1)   /* volumetric_rendering.py:59  rgb += 1 - sum(w) */
#define CNERF_F_LAST_BACK (1u << 2)    /* volumetric_rendering.py:53  w[last] += 1 - sum(w) */
#define CNERF_F_SOFTPLUS (1u << 3)     /* clamp_mode == "softplus" (else "relu"), volumetric_rendering.py:41-44 */
#define CNERF_F_SIGMOID_RGB (1u << 4)  /* siren.py:1227-1234  sigmoid on channels 0..2 of the head */
#define CNERF_F_INPUT_XYZ (1u << 5)    /* siren.py:1158  layer 0 sees features || world xyz (TALLSIREN_dgx) */
#define CNERF_F_RESERVED6 (1u << 6)    /* reserved (ABI v4-v5: selected an experimental kernel variant that was measured slower and
                                          removed in v6); ignored */
#define CNERF_F_NO_VOLUME (1u << 7)    /* siren.py:1172-1224 (SHORTSIREN, ABI v10): the network reads no feature volume -- layer 0 sees the sample's
                                          world xyz (K = 3), FiLM frequencies / phases come per image from the caller.  Requires C == 0 and
                                          n_levels == 0 (V is not read); layer kinds FILM / SINE / RES (PFILM: CNERF_EINVAL); not together with
                                          CNERF_F_INPUT_XYZ (CNERF_EINVAL).  `vols` / `grad_vols` arguments may be NULL and are never dereferenced,
                                          cnerf_workspace_bytes reports fvol_cl = 0, no backward scatters anything, and the position gradient of
                                          cnerf_field_query_backward is the xyz term alone (no clamp: it is non-zero outside the 1.2 cube).
                                          All three precisions and both backward precisions (dropout: fp32 only, as everywhere).  fp32: layer 0 runs
                                          as three fp32 fmas per output channel on the vector units, no K = 32 MFMA tile; fp16x3 / fp16: as the
                                          first weight unit on the zero-padded xyz tile.  No kernel looks anything up or keeps loads in flight
                                          across tiles; the half-precision backward reserves no input-gradient rows and launches no patch scatter.
                                          cnerf_gather_features / cnerf_scatter_features / cnerf_feature_points_grad refuse the flag. */

/* cnerf_cfg.precision */
#define CNERF_PREC_FP32 0   /* v_mfma_f32_32x32x2_f32: exact fp32 fmaf chains */
#define CNERF_PREC_FP16 1   /* plain fp16 products, fp32 accumulation (one v_mfma_f32_32x32x16_f16 per 16 k-values; weights pre-scaled per
                             * matrix by a power of two, activations rounded to nearest): the numerics class of the reference's GPU path
                             * (torch.cuda.amp.autocast, utils.py:327,643) and of BASELINE config 5; NOT inside the 1e-4 gate (measured
                             * ~1e-3 on rgb / sigma: tests/test_gpu_parity.py::test_single_pass_fp16) -- use fp16x3 for that */
#define CNERF_PREC_FP16X3 2 /* every fp32 operand split into two fp16 parts (22 significant bits), three fp16 MFMAs per product
                             * with fp32 accumulation, weights pre-scaled per matrix by a power of two: fp32-level accuracy
                             * (same parity gate) at 3/16 of the fp32 matrix time; forward and the activation-storing re-run of the
                             * backward; FiLM / sine / residual layers (not the per-point FiLM family) */

/* layer kinds of the field network (siren.py:146-230) */
#define CNERF_LAYER_FILM 0 /* y = sin(freq * (W x + b) + phase), freq/phase per image */
#define CNERF_LAYER_SINE 1 /* y = sin(W x + b) */
#define CNERF_LAYER_RES 2  /* y = sin(x + W2 sin(W1 x + b1) + b2) */
#define CNERF_LAYER_PFILM 3 /* y = sin(freq(p) * (W x + b) + phase(p)): per-point FiLM from the mapping MLP of the looked-up
                               feature (siren.py:163-177, 81-101); all layers of the network must be of this kind, layer 0
                               then reads the world position (K = 3) and the features feed the mapping MLP only.  All three
                               precisions (ABI v7: CNERF_PREC_FP16X3 / CNERF_PREC_FP16 in csrc/field_pw16.hip) */

typedef struct cnerf_cfg {
    int32_t B;            /* images in this call */
    int32_t R;            /* img_size */
    int32_t S;            /* num_steps (coarse samples per ray) */
    int32_t V;            /* feature volume side (level 0) */
    int32_t C;            /* feature channels over all levels; input width of layer 0 = C (+3 with CNERF_F_INPUT_XYZ);
                             0 with CNERF_F_NO_VOLUME (input width 3) */
    int32_t H;            /* hidden width (multiple of 32, <= 256) */
    int32_t L;            /* number of entries in layer_kind */
    int32_t layer_kind[CNERF_MAX_LAYERS];
    float ray_start;      /* forward(ray_start) */
    float ray_end;        /* forward(ray_end) */
    float voxel_length;   /* 1.2, siren.py:555 */
    float noise_std;      /* kwargs["nerf_noise"] */
    uint32_t flags;       /* CNERF_F_* */
    double fov_deg;       /* forward(fov), degrees; kept in double because the reference takes tan() of the
                             Python float before rounding the focal length to fp32 (volumetric_rendering.py:85-87) */
    int32_t n_levels;     /* feature volumes looked up and concatenated (0 or 1: the single volume V, C) */
    int32_t level_V[CNERF_MAX_LEVELS]; /* side of level i */
    int32_t level_C[CNERF_MAX_LEVELS]; /* channels of level i (multiple of 32); sum = C */
    int32_t precision;    /* CNERF_PREC_*: arithmetic of the MLP products in the FORWARD kernels */
    /* In-kernel random draws (ABI v4).  philox != 0: every draw whose tensor in cnerf_rng is NULL is generated inside the
     * kernels by Philox4x32-10 with key = philox_seed and counter = (element index in the whole call, stream, philox_offset) --
     * stream 0 u_strat (B,P,S), 1 eps_coarse (B,P,S), 2 u_fine (B,P,S), 3 eps_final (B,P,S') indexed in sorted order; the noise
     * streams only when noise_std != 0.  A pure function of (seed, offset, index): the backward entry points given the same cfg
     * see the same draws, no tensor travels.  Use a fresh philox_offset per call.  philox == 0: NULL tensors mean "no jitter /
     * no noise" as before (and u_fine is required).  cnerf_philox_fill materialises a stream; oracle/philox.py is its NumPy twin. */
    uint32_t philox;
    uint32_t philox_offset;
    uint64_t philox_seed;
    /* Dropout in training mode (ABI v5): nn.Dropout(p) behind the sine of every FiLMLayer / SirenLayer / PointwiseFiLMLayer
     * (siren.py:158-159,175-176,197-198; residual blocks have none).  drop_p in [0,1), 0 = off (eval mode).  Kept values are
     * multiplied by 1 / (1 - p) like ATen does.  Keep decisions per (dropout layer d, point, channel): the bytes of
     * cnerf_rng.drop_coarse / drop_fine where given, else Philox4x32-10 under (philox_seed, philox_offset) -- whether or not
     * `philox` is set -- stream 4 (coarse pass), 5 (fine pass), 6 (cnerf_field_forward), one block per 4 channels: counter index
     * ((point index in the whole call * n_drop + d) * H + c) / 4, word c % 4 keeps iff >= round(p * 2^32); n_drop = number of
     * layers that are not residual blocks.  The backward entry points given the same cfg (and masks) see the same decisions.
     * Precision fp32 only (CNERF_EINVAL otherwise). */
    float drop_p;
    uint32_t reserved0;
} cnerf_cfg;

/* Feature volumes, channel-last: level[i] is (B, V_i, V_i, V_i, C_i).  HOST struct of device pointers.  The gradient
 * twin of the backward has the same shapes and is accumulated into.  CNERF_F_NO_VOLUME: there are none; every `vols` /
 * `grad_vols` argument below may then be NULL. */
typedef struct cnerf_volumes {
    const float* level[CNERF_MAX_LEVELS];
} cnerf_volumes;
typedef struct cnerf_grad_volumes {
    float* level[CNERF_MAX_LEVELS];
} cnerf_grad_volumes;

/* Raw parameters of the field network, exactly as the nn.Module holds them (row-major [out][in]).
 * For a RES layer i: w[i]/b[i] = fc1, w2[i]/b2[i] = fc2.  Replaces the state the reference keeps in
 * siren.network[i].layer.{weight,bias} / .fc1 / .fc2 and siren.final_layer (siren.py:611-625). */
typedef struct cnerf_field_params {
    const float* w[CNERF_MAX_LAYERS];
    const float* b[CNERF_MAX_LAYERS];
    const float* w2[CNERF_MAX_LAYERS];
    const float* b2[CNERF_MAX_LAYERS];
    const float* w_final; /* [4][H] */
    const float* b_final; /* [4] */
    /* per-point FiLM family only (siren.mapping_network.network.{0,2}, siren.py:81-101) */
    const float* map_w1;  /* [256][C]      */
    const float* map_b1;  /* [256]         */
    const float* map_w2;  /* [2*L*H][256]  freq rows first, then phase rows */
    const float* map_b2;  /* [2*L*H]       */
} cnerf_field_params;

/* The four random tensors the reference draws, in its draw order; any may be NULL (then: cnerf_cfg.philox):
 *   u_strat    (B,P,S)   uniform, stratified jitter          volumetric_rendering.py:106  (NULL -> 0.5, no jitter)
 *   eps_coarse (B,P,S)   normal, density noise, coarse pass  volumetric_rendering.py:39   (NULL -> 0)
 *   u_fine     (B,P,S)   uniform, inverse-CDF draws          volumetric_rendering.py:319  (required if hierarchical)
 *   eps_final  (B,P,S')  normal, final pass, S' = 2S or S    volumetric_rendering.py:39   (NULL -> 0)
 * eps_final is indexed in SORTED sample order, as the reference adds its noise after the merge.
 *   fine_z     (B,P,S)   test hook, normally NULL: depths that REPLACE the resampled ones for the fine pass and the merge
 *                        (the resampling still runs and fills aux).  The field is chaotic in position, so parity of the
 *                        fine pass / merge / final composite is pinned by forcing the reference's own fine depths.
 *   drop_coarse, drop_fine (n_drop, B, P*S, H) uint8, 1 = keep: dropout decisions of the two field passes (cnerf_cfg.drop_p;
 *                        normally NULL: Philox).  What F.dropout drew in the reference, layer after layer, for tests. */
typedef struct cnerf_rng {
    const float* u_strat;
    const float* eps_coarse;
    const float* u_fine;
    const float* eps_final;
    const float* fine_z;
    const uint8_t* drop_coarse;
    const uint8_t* drop_fine;
} cnerf_rng;

/* Optional intermediate outputs (each may be NULL).  Shapes per image-major layout:
 *   coarse_points (B,P,S,3) coarse_z (B,P,S) coarse_rgb_sigma (B,P,S,4) coarse_weights (B,P,S)
 *   cdf (B,P,S-1) inds (B,P,S) int32   fine_z (B,P,S) fine_rgb_sigma (B,P,S,4)
 *   sort_idx (B,P,2S) int32 (index into cat[fine, coarse])   final_weights (B,P,S')   fine_points (B,P,S,3) */
typedef struct cnerf_aux {
    float* coarse_points;
    float* coarse_z;
    float* coarse_rgb_sigma;
    float* coarse_weights;
    float* cdf;
    int32_t* inds;
    float* fine_z;
    float* fine_rgb_sigma;
    int32_t* sort_idx;
    float* final_weights;
    float* fine_points; /* (B,P,S,3) */
    /* Optional profiling hooks (HOST handles): hipEvent_t created by the caller, recorded on the call's stream
     * immediately before / after the field kernel of the coarse pass ([0],[1]) and of the fine pass ([2],[3]).
     * NULL entries are skipped.  bench.py uses them to time the dominant kernel inside the timed region. */
    void* field_events[4];
    /* Optional (ABI v4), precision CNERF_PREC_FP16X3 only: keep the activations of the two field passes for the half-precision
     * backward instead of re-computing them there -- act16[0] coarse pass, act16[1] fine pass; each {feat (T, n_in, 32, 32),
     * h (n_mats, T, H/32, 32, 32), c (same)} fp16 in the TB16 layout over ALL images of the call (T = B * ceil(R*R*S / 32)).
     * 4 KiB per sample point at H = 256, 4 layers: sized for the 288 GB of HBM of an MI355X (batch 8 at 128x128x(64+64): 69 GB).
     * All-NULL entries: nothing is kept. */
    struct {
        void* feat;
        void* h;
        void* c;
        void* amax; /* ABI v7, CNERF_LAYER_PFILM networks only: (L, T * 32) floats; their feat is (T, 2, 32, 32), h L slabs (T, H/32, 32, 32)
                       then m (T, 8, 32, 32), c 3 L slabs -- 16.5 KiB per sample point and pass at H = 256, L = 8 */
    } act16[2];
} cnerf_aux;

int cnerf_abi_version(void);
/* out[i] = draw i of stream `stream_id` under (seed, offset): uniform in [0,1) (normal == 0) or standard normal (normal != 0),
 * exactly what the kernels generate when cnerf_cfg.philox is set.  Replaces torch.rand / torch.randn at
 * volumetric_rendering.py:39,106,319 for hosts that want the tensors. */
int cnerf_philox_fill(uint64_t seed, uint32_t offset, uint32_t stream_id, int64_t n, int32_t normal, float* out, void* stream);
/* Host string describing the last error raised on the calling thread ("" if none). */
const char* cnerf_last_error(void);

/* Validates cfg and returns the byte sizes the caller must provide:
 *   packed   : packed field weights written by cnerf_pack_field
 *   fvol_cl  : channel-last copy of the feature volume written by cnerf_fvol_channel_last (0 with CNERF_F_NO_VOLUME)
 *   fwd_ws   : scratch of cnerf_render_forward (coarse / fine rgb_sigma and depths, and the folded FiLM constants of the call:
 *              per image, matrix and channel  freq / 2 pi  and  (freq * bias + phase) / 2 pi, and the layer weights with their rows scaled
 *              by freq / 2 pi per image, prepared once for both field passes in fp32 precision) */
int cnerf_workspace_bytes(const cnerf_cfg* cfg, size_t* packed, size_t* fvol_cl, size_t* fwd_ws);

/* (B,C,V,V,V) channel-first, as unet3d emits it (generators/unet3d.py) -> (B,V,V,V,C) channel-last, so that one
 * trilinear corner is one contiguous C*4-byte line.  Replaces the layout F.grid_sample reads (siren.py:561-567). */
int cnerf_fvol_channel_last(int32_t B, int32_t C, int32_t V, const float* fvol_cf, float* fvol_cl, void* stream); /* C % 32 == 0 */
/* Transpose of the above (used for the gradient of the feature volume). */
int cnerf_fvol_channel_first(int32_t B, int32_t C, int32_t V, const float* fvol_cl, float* fvol_cf, void* stream);

/* Re-orders nn.Linear weights into MFMA A-operand order (see DESIGN.md "packed weights").  params is a HOST struct
 * of device pointers. */
int cnerf_pack_field(const cnerf_cfg* cfg, const cnerf_field_params* params, float* packed, void* stream);

/* Trilinear lookup only: points (B,n,3) world -> feat (B,n,C).  Replaces F.grid_sample + permute
 * (siren.py:555-571, K4/K5 of SURVEY.md 2.1).  This is the unfused "sample pass" kernel the HBM roofline is quoted on. */
int cnerf_gather_features(const cnerf_cfg* cfg, const float* fvol_cl, const float* points, int64_t n_per_image,
                          float* feat, void* stream);

/* Field network at explicit points: points (B,n,3) -> rgb_sigma (B,n,4).
 * Replaces <SIREN>.forward(points, z, img_size, num_steps) (siren.py:637-668 and siblings; extract_shapes.py:63-69).
 * freq/phase: (B, n_film*H) with freq already *15+30 (siren.py:650), NULL when the network has no FiLM layer. */
int cnerf_field_forward(const cnerf_cfg* cfg, const cnerf_volumes* vols, const float* packed, const float* freq,
                        const float* phase, const float* points, int64_t n_per_image, float* rgb_sigma, void* stream);

/* Alpha compositing of n samples per ray: rgb_sigma (rays,n,4), z (rays,n), eps (rays,n) or NULL ->
 * rgb (rays,3), dist (rays), weights (rays,n) (each output may be NULL).
 * Replaces fancy_integration (volumetric_rendering.py:18-70).  Uses cfg->noise_std and flags. */
int cnerf_composite(const cnerf_cfg* cfg, int64_t rays, int32_t n, const float* rgb_sigma, const float* z,
                    const float* eps, float* rgb, float* dist, float* weights, void* stream);

/* Inverse-CDF resampling: z, weights, u (rays,S) -> fine_z (rays,S); optional inds (rays,S) int32, cdf (rays,S-1).
 * Replaces generators.py:123-137 + sample_pdf (volumetric_rendering.py:297-342). */
int cnerf_resample(int64_t rays, int32_t S, const float* z, const float* weights, const float* u, float* fine_z,
                   int32_t* inds, float* cdf, void* stream);

/* The whole path: ImplicitGenerator3d.forward (generators.py:33-187).
 *   cam2world (B,4,4) row-major;  pixels (B,3,R,R) = 2*rgb-1;  depth (B,R,R).  aux may be NULL. */
int cnerf_render_forward(const cnerf_cfg* cfg, const cnerf_volumes* vols, const float* packed, const float* freq,
                         const float* phase, const float* cam2world, const cnerf_rng* rng, float* pixels,
                         float* depth, const cnerf_aux* aux, void* workspace, void* stream);

/* ---- backward (autograd twin of cnerf_render_forward; gradients flow to the field parameters, freq/phase and the
 * feature volume, never to cam2world or the sample positions: generators.py:57,111 run them under no_grad.  This grid render's
 * backward gives no position gradient; a field query's does (cnerf_field_query_backward below), and so does a render of caller-given
 * rays: cnerf_render_rays_backward returns d loss / d origins and d loss / d directions) ----------
 *
 * Step 1  cnerf_merge_composite_backward: d(pixels, depth) -> d(rgb_sigma) of the coarse and the fine samples.
 * Step 2  cnerf_field_backward per pass (coarse, fine) and per chunk of images: re-runs the field forward storing the
 *         activations, back-propagates through the MLP on the MFMA units, scatter-adds d(feature volume) with fp32
 *         atomics, and leaves row-major activation / gradient matrices in the caller's chunk buffers:
 *             act_feat (n,32k)  x0 = layer-0 input tiles            act_go (n,4)   d/d head pre-activation
 *             act_h (L,n,H)     x_l = sin(arg_l)                    act_g  (L,n,H) d/d arg_l
 *             act_c (L,n,H)     cos(arg_l)                          (n = images_in_chunk * points_per_image)
 *         The parameter gradients are then plain GEMMs / column sums over these matrices (rocBLAS territory):
 *             dWarg_l = act_g[l]^T x_{l-1};  dW_l = diag(freq_l) dWarg_l;  db_l = freq_l * colsum(act_g[l])
 *             dphase_l = colsum(act_g[l]);   dfreq_l = rowsum(W_l * dWarg_l) + b_l * dphase_l   (per image)
 *             dW_head = act_go^T x_L;        db_head = colsum(act_go)
 * A residual block owns two consecutive slabs of act_h / act_c / act_g (fc1 then fc2); L in the shapes above then counts
 * slabs:  dW_fc1 = act_g[s]^T x_in, dW_fc2 = act_g[s+1]^T act_h[s].
 *
 * Per-point FiLM family (CNERF_LAYER_PFILM, TALLSIREN siren.py:232-331:  m = LeakyReLU_0.2(Wm1 feat + bm1), [f | p] = Wm2 m + bm2,
 * y_l = sin((15 f_l + 30) (W_l y_{l-1} + b_l) + p_l), y_-1 = xyz): the same call with larger chunk buffers --
 *             act_feat (n,32)                  looked-up feature            act_go (n,4)  d/d head pre-activation
 *             act_h  L (n,H) slabs of y_l, then m (n,256)                    (L*n*H + n*256 floats)
 *             act_c  3L (n,H) slabs: per layer cos(arg), cos*freq, cos*15*pre   (scratch of the call: nothing reads it afterwards)
 *             act_g  L (n,H) slabs of g_pre_l = d/d (W_l y_{l-1} + b_l), then G (n, 2*L*H) = d/d (Wm2 m + bm2), row by row in
 *                    that Linear's output order [f of layers 0..L-1 | p of layers 0..L-1]           (3*L*n*H floats)
 *         and no volume scatter (grad_vols is not touched).  What remains are products over those matrices, all of them behind ONE
 *         further call per chunk, cnerf_pfilm_backward_finish (csrc/pfilm_finish.hip; below):
 *             dW_l = act_g[l]^T y_{l-1} (layer 0: y_-1 = the sample positions, K = 3), db_l = colsum(act_g[l]), the head's dW / db,
 *             dWm2 = G^T m, dbm2 = colsum(G), g_m = (G Wm2) * (m > 0 ? 1 : 0.2), dWm1 = g_m^T feat, dbm1 = colsum(g_m),
 *             d feat = g_m Wm1, scattered into the feature volume's gradient with the trilinear weights of the sample positions. */

/* packed_t: transposed packed weights for the backward; bytes via cnerf_backward_bytes. */
int cnerf_backward_bytes(const cnerf_cfg* cfg, size_t* packed_t);
int cnerf_pack_field_transposed(const cnerf_cfg* cfg, const cnerf_field_params* params, float* packed_t, void* stream);

/* saved tensors are the forward's coarse/fine rgb_sigma and z (cnerf_aux); fine_* may be NULL when not hierarchical.
 * grad_depth may be NULL.  Outputs grad_coarse / grad_fine: (B,P,S,4). */
int cnerf_merge_composite_backward(const cnerf_cfg* cfg, const float* coarse_rgb_sigma, const float* coarse_z,
                                   const float* fine_rgb_sigma, const float* fine_z, const float* eps_final,
                                   const float* grad_pixels, const float* grad_depth, float* grad_coarse,
                                   float* grad_fine, void* stream);

/* pass: 0 = coarse samples (needs u_strat as in the forward), 1 = fine samples (needs fine_z), 2 = explicit points:
 * the u_strat argument then carries points (B, R*R*S, 3) (backward of cnerf_field_forward).  Images [image0,
 * image0 + n_images) of the call described by cfg.  All per-image inputs are the FULL tensors of the forward (the
 * function offsets them); grad_rgb_sigma / saved_rgb_sigma are the (B,P,S,4) tensors of that pass; grad_vols are the
 * full gradient volumes, accumulated into (zero them first).  act_* are chunk buffers for n_images images; act_feat is
 * (n, 32 * input tiles): the concatenated looked-up features (and xyz, zero padded) that layer 0 saw.
 * `packed` is in the layout of cfg->precision (the activation-storing forward runs in that precision); packed_t is always
 * the fp32 transposed layout (the gradient chain is fp32).  drop_mask: cnerf_rng.drop_coarse / drop_fine of that pass (the FULL
 * tensor) or NULL; with cfg->drop_p > 0 the stored sine and cosine rows carry the dropout factor, so the chain, the weight
 * reductions and the scatter are the ones of the eval-mode network. */
int cnerf_field_backward(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const cnerf_volumes* vols,
                         const float* packed, const float* packed_t, const float* freq, const float* phase,
                         const float* cam2world, const float* u_strat, const float* fine_z,
                         const float* grad_rgb_sigma, const float* saved_rgb_sigma, float* act_feat, float* act_h,
                         float* act_c, float* act_g, float* act_go, const cnerf_grad_volumes* grad_vols, const uint8_t* drop_mask,
                         void* stream);

/* Weight-gradient reduction over a chunk written by cnerf_field_backward:  dW[b] (H,K) += g_arg[b]^T x[b],
 * colsum[b] (H) += sum over points of g_arg[b], per image b < n_images; g_arg (n_images, n_per_image, H) = act_g of one
 * matrix, x (n_images, n_per_image, K) = that matrix' input (act_feat for layer 0, act_h of the previous matrix otherwise),
 * K a multiple of 32.  From these the host forms dW, db, dfreq, dphase (autograd of FiLMLayer / SirenLayer,
 * siren.py:146-199).  Both outputs are accumulated into (zero them first). */
int cnerf_weight_grad(int32_t n_images, int64_t n_per_image, int32_t H, int32_t K, const float* g_arg, const float* x, float* dW,
                      float* colsum, void* stream);

/* Adjoint of cnerf_gather_features: grad_fvol_cl (B,V,V,V,32) += scatter of grad_feat (B,n,32) with the trilinear weights of
 * points (B,n,3).  Autograd twin of F.grid_sample (siren.py:555-571) for hosts that evaluate the MLP gradients themselves
 * (the per-point FiLM family, siren.py:232-331). */
int cnerf_scatter_features(const cnerf_cfg* cfg, const float* points, int64_t n_per_image, const float* grad_feat,
                           float* grad_fvol_cl, void* stream);

/* ---- half-precision backward (ABI v4): the counterpart of the reference's fp16 autocast training (utils.py:643-711) ------
 * Activations and their gradients travel in fp16, every sum is fp32.  Buffers use the TB16 layout: a matrix with one row per
 * sample point and 32 * CT channels is stored per 32-point tile (the field kernels' work unit: image b, tile k of
 * tiles_per_image = ceil(R*R*S / 32), T = b * tiles_per_image + k) and per 32-channel tile as a dense 32 x 32 fp16 block:
 *     element (T, t, j, c) -> fp16 index ((T * CT + t) * 32 + j) * 32 + c.
 * Rows past the end of an image are rows of their own (gradient rows there are written as zeros). */

/* dW[b] (n_rows, 32 * x_ct) += G[b]^T X[b] and colsum[b] (n_rows) += column sums of G[b], per image b < n_images, over the
 * tiles of that image; G: TB16 with g_ct channel tiles of which the first ceil(n_rows / 32) are used (n_rows = 4 for the head:
 * dW_head = go'^T x_L), X: TB16 with x_ct <= 8 channel tiles.  G holds scale * g; inv_scale (DEVICE scalar, may be NULL = 1)
 * undoes it.  Outputs are accumulated into (zero them first); colsum may be NULL.  Autograd of nn.Linear inside
 * FiLMLayer / SirenLayer (siren.py:146-199) like cnerf_weight_grad, on v_mfma_f32_32x32x16_f16. */
int cnerf_weight_grad16(int32_t n_images, int64_t tiles_per_image, int32_t n_rows, int32_t g_ct, int32_t x_ct, const void* G,
                        const void* X, float* dW, float* colsum, const float* inv_scale, void* stream);

/* Packed operands of the half-precision gradient chain: every W_l^T (and the head's) as fp16 MFMA fragments, each matrix
 * pre-scaled by a power of two, plus their inverse scales.  Bytes via cnerf_backward16_bytes.  FiLM, plain-sine and residual-block
 * networks: a residual block is two matrices -- fc1, fc2 -- of every per-matrix array below; the per-point FiLM family packs the
 * operands of its own chain (csrc/chain_pw16.hip) behind the same two calls. */
int cnerf_backward16_bytes(const cnerf_cfg* cfg, size_t* packed16);
int cnerf_pack_field_chain16(const cnerf_cfg* cfg, const cnerf_field_params* params, void* packed16, void* stream);

/* ---- the whole backward in ONE call (ABI v6) --------------------------------------------------------------------------
 * Autograd twin of cnerf_render_forward for hosts without an autograd engine of their own (and the path the PyTorch mirror
 * takes): given d loss / d pixels and d loss / d depth it runs the steps above -- cnerf_merge_composite_backward, then per
 * pass (coarse, fine) and per chunk of images the activation-storing re-run of the forward (unless the forward kept its
 * activations: aux->act16), the gradient chain, the volume scatter, one weight reduction per matrix -- and finishes what the
 * round-2 ABI left to the host: dW_l = diag(freq_l) dWarg_l, db_l, dfreq_l, dphase_l per image, the head's dW / db.
 * Replaces loss.backward() through ImplicitGenerator3d.forward (utils.py:638-711; generators.py:33-187 under autograd).
 *
 *   backward_precision  CNERF_PREC_FP32: exact fp32 chain and weight reductions (re-run in cfg->precision);
 *                       CNERF_PREC_FP16: fp16 operands, fp32 sums (csrc/bwd16.hip, cnerf_weight_grad16; cfg->precision must
 *                       be CNERF_PREC_FP16X3).  Per-point FiLM networks: grads->map_* receive the mapping network's gradients, all of
 *                       grads' buffers of the family are required; CNERF_PREC_FP16 (ABI v7) is csrc/chain_pw16.hip, CNERF_PREC_FP32 needs
 *                       cfg->precision = CNERF_PREC_FP32 and runs per pass and chunk what the stage calls spell: cnerf_field_backward,
 *                       then cnerf_pfilm_backward_finish on the positions the re-run wrote (the forward need not keep any), into a
 *                       workspace of the five chunk matrices above, (n,3) positions and the stage's workspace and packed_map.
 *   params              the raw parameters (dfreq needs W_l and b_l);  packed: cnerf_pack_field in cfg->precision;
 *   packed_bwd          cnerf_pack_field_transposed (fp32 backward) or cnerf_pack_field_chain16 (fp16 backward).
 *   saved               the forward's coarse / fine rgb_sigma and z (cnerf_aux of that call; fine_* NULL when not hierarchical).
 *   rng                 the forward's cnerf_rng -- u_strat, eps_final, dropout masks; Philox draws follow cfg as in the forward.
 *   act16               the activations the forward kept (cnerf_aux.act16, fp16 backward only) or NULL: re-computed per chunk.
 *   grads               per parameter a buffer of the parameter's shape, ACCUMULATED INTO (zero them first); NULL entries are
 *                       skipped.  grad_freq / grad_phase (B, n_film * H), grad_vols (shapes of vols): accumulated into as well.
 *   images_per_chunk    images whose activation / gradient buffers live in the workspace at a time (1..B; with act16 given
 *                       all B).  workspace: cnerf_backward_workspace_bytes(cfg, backward_precision, images_per_chunk, act16 != NULL).
 *   saturated           optional DEVICE uint32 (zero it first), fp16 backward: incremented once per (tile, matrix) in which a stored
 *                       gradient exceeded fp16's range and was clamped -- the per-matrix scale comes from a SAMPLED maximum
 *                       (every 16th tile group once there are >= 32768 of them); non-zero means: repeat in fp32. */
typedef struct cnerf_field_param_grads {
    float* w[CNERF_MAX_LAYERS];
    float* b[CNERF_MAX_LAYERS];
    float* w2[CNERF_MAX_LAYERS];
    float* b2[CNERF_MAX_LAYERS];
    float* w_final;
    float* b_final;
    /* per-point FiLM family only (ABI v7): gradients of siren.mapping_network.network.{0,2} */
    float* map_w1; /* [256][C]      */
    float* map_b1; /* [256]         */
    float* map_w2; /* [2*L*H][256]  */
    float* map_b2; /* [2*L*H]       */
} cnerf_field_param_grads;

typedef struct cnerf_saved {
    const float* coarse_rgb_sigma; /* (B,P,S,4) */
    const float* coarse_z;         /* (B,P,S)   */
    const float* fine_rgb_sigma;   /* (B,P,S,4) or NULL */
    const float* fine_z;           /* (B,P,S) or NULL: the depths the fine pass used */
} cnerf_saved;

/* Half-precision backward, feature-volume gradient: the ray passes' input-tile gradients go through the workspace (128 B per point) and
 * are added to grad_vols pre-reduced per 8 x 8-pixel patch (csrc/scatter_patch.hip).  Environment CNERF_SCATTER=chain makes the
 * gradient chain add them itself (A/B runs and tests only): the same addends in another order. */
int cnerf_backward_workspace_bytes(const cnerf_cfg* cfg, int32_t backward_precision, int32_t images_per_chunk, int32_t have_act16,
                                   size_t* bytes);

/* Stage entry of that patch scatter, for hosts that sequence the stages themselves -- cnerf_render_backward runs it per pass and chunk
 * behind the half-precision chain -- and what tests/test_gpu_scatter_patch.py holds to float64 voxel by voxel (added in ABI v10 without
 * a version change: no struct changed):
 * grad_vols[level] (images [image0, image0 + n_images)) += the trilinear scatter of gin with the weights of the sample positions of
 * ray pass `pass` (0 coarse: u_strat or NULL = Philox; 1 fine: fine_z), formed as cnerf_field_backward forms them.
 * gin: (feature input tiles of the network in layer-0 order, n_images * R*R*S, 32) fp32, the rows of the chunk's first image first;
 * tile t of level i adds to channels [32 t, 32 t + 32) of that level; an xyz tile (CNERF_F_INPUT_XYZ) has no rows.  cam2world, u_strat,
 * fine_z and grad_vols are the FULL tensors of the call described by cfg (the function offsets them); gin is 16-byte aligned.
 * CNERF_EINVAL and no launch: pass 2 (explicit points are no pixel patches), CNERF_F_NO_VOLUME, a NULL cam2world / gin / grad_vols /
 * level / fine_z of the fine pass, an image range outside [0, B). */
int cnerf_scatter_patches(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const float* cam2world,
                          const float* u_strat, const float* fine_z, const float* gin, const cnerf_grad_volumes* grad_vols, void* stream);

/* Stage entry of the half-precision gradient chain (csrc/bwd16.hip, chain16_kernel; FiLM / plain-sine / residual networks), for hosts
 * that sequence the stages themselves and what tests/test_gpu_chain16.py holds to float64 row by row (added in ABI v10 without a version
 * change: no struct changed).  On the caller's buffers it runs the launches cnerf_render_backward runs per pass and chunk between the
 * storing forward and the reductions -- the head's scale from the largest |grad_rgb_sigma| of the chunk, the chain's dry run over the
 * sampled tile groups, the per-slab scales, the chain -- for images [image0, image0 + n_images) of ray pass `pass` (0 / 1 / 2 as
 * cnerf_field_backward; pass 2: u_strat carries the points (B, R*R*S, 3)); tiles = n_images * ceil(R*R*S / 32), n_mats = the network's
 * matrices before the head (a residual block: fc1, fc2).
 *   packed16        cnerf_pack_field_chain16.  freq: the call's FULL (B, n_film * H) tensor (NULL without FiLM layers).
 *   cam2world, u_strat, fine_z: the FULL tensors; the chain forms the sample positions of every tile (it scatters with them when gin is NULL).
 *   grad_rgb_sigma, saved_rgb_sigma: the FULL (B, R*R*S, 4) tensors of the pass.
 *   cos16           cos(arg) of every slab for the chunk's tiles, fp16, fragment-major (COS16 of csrc/bwd16.hpp):
 *                   element (slab m, tile T, channel 32 t + 8 g + 4 h + e of point j) -> ((((m * tiles + T) * NT + t) * 4 + g) * 64 + j + 32 h) * 4 + e.
 *   group_step      0: the render's rule (every (groups / 2048)-th group of four tiles, 1..16); k >= 1: the dry run samples every k-th.
 * Outputs:
 *   g16             TB16 (n_mats, tiles, NT, 32, 32): d loss / d (sine argument) of slab m times scales[2 m]; rows past an image's end are 0.
 *   go16            TB16 (tiles, 1, 32, 32): d loss / d (head pre-activation) times scales[2 n_mats] in channels 0..3, zeros elsewhere.
 *   scales          2 (n_mats + 1) floats: {S, 1 / S} per slab, then the head's.
 *   gmax            n_mats + 2 words, the bits of non-negative floats: per slab the largest sampled |gradient| in true units, the largest
 *                   sampled head gradient, the largest |grad_rgb_sigma| of the chunk.
 *   gin             (feature input tiles, n_images * R*R*S, 32) fp32, true units, the layout cnerf_scatter_patches reads -- or NULL, and
 *   grad_vols       (the FULL gradient volumes) is ACCUMULATED INTO by the chain's own atomics.  Exactly one of the two for a network
 *                   with a volume; neither is touched for CNERF_F_NO_VOLUME.
 *   saturated       optional, as in cnerf_render_backward: += 1 per (tile, slab) whose stored gradients were clamped to fp16's range.
 * CNERF_EINVAL and no launch: per-point FiLM networks, cfg->precision != CNERF_PREC_FP16X3, pass outside 0..2, an image range outside
 * [0, B), group_step < 0, a NULL required argument (freq of a FiLM network, cam2world of a ray pass, fine_z of the fine pass, the points
 * of pass 2 among them), both or neither of gin / grad_vols for a network with a volume, a NULL level of grad_vols. */
int cnerf_field_chain16(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const void* packed16, const float* freq,
                        const float* cam2world, const float* u_strat, const float* fine_z, const float* grad_rgb_sigma,
                        const float* saved_rgb_sigma, const void* cos16, int32_t group_step, void* g16, void* go16, float* scales, uint32_t* gmax,
                        float* gin, const cnerf_grad_volumes* grad_vols, uint32_t* saturated, void* stream);

/* Stage entry of the activation-storing re-run in front of that chain (csrc/field_h3.hip, field_h3_kernel<NT, STORE_TB16, HAS_RES, WF = 0>;
 * FiLM / plain-sine / residual networks), for hosts that sequence the stages themselves and what tests/test_gpu_store16.py holds to
 * float64 row by row (added in ABI v10 without a version change: no struct changed).  On the caller's buffers it runs the ONE launch
 * cnerf_render_backward runs per pass and chunk when the forward kept no activations: the field pass over images [image0, image0 +
 * n_images) of `pass` (0 / 1 / 2 as cnerf_field_backward; pass 2: u_strat carries the points (B, R*R*S, 3)) again on the fp16x3 kernel,
 * storing what the chain and the weight reductions read.  vols, freq, phase, cam2world, u_strat, fine_z are the FULL tensors of the call
 * described by cfg (the function offsets them); packed: cnerf_pack_field in CNERF_PREC_FP16X3.  tiles = n_images * ceil(R*R*S / 32),
 * NT = H / 32, n_in = layer 0's 32-wide input tiles (per level its channel tiles, then the xyz tile), n_mats as for cnerf_field_chain16.
 * Outputs, fp16, 16-byte aligned, the chunk's first image first (tile T = image of the chunk * ceil(R*R*S / 32) + tile of the image):
 *   feat            TB16 (tiles, n_in, 32, 32): layer 0's input rows, fp16(clamp(x, +-65504)); an xyz tile holds the position in columns
 *                   0..2 and zeros in 3..31.
 *   h               TB16 (n_mats, tiles, NT, 32, 32): sin(arg) of every slab; channel 32 t + k of point j of tile T ->
 *                   (((m * tiles + T) * NT + t) * 32 + j) * 32 + k.
 *   c               COS16 (n_mats, tiles, NT, 4, 64, 4): cos(arg), the layout of cnerf_field_chain16's cos16.
 *   rgb_sigma       (n_images * R*R*S, 4) fp32: the head's output (cnerf_render_backward discards it into a scratch buffer).
 * Rows past an image's end (the padded lanes of an image's last tile) hold the rows of the image's LAST point, in feat, h and c alike:
 * cnerf_weight_grad16 multiplies them by the chain's zero gradient rows, so they must be finite whatever the buffer held before.  A wave
 * without a tile (the tiles of an image are worked on in groups of four) stores nothing: the buffers have no block for it, and nothing
 * outside the chunk's tiles is written.
 * CNERF_EINVAL and no launch: per-point FiLM networks, cfg->precision != CNERF_PREC_FP16X3, drop_p != 0 (dropout exists in fp32 only),
 * pass outside 0..2, an image range outside [0, B), a NULL required argument (vols of a network with a volume or one of its levels, packed,
 * freq / phase of a FiLM network, cam2world of a ray pass, fine_z of the fine pass, the points of pass 2, an output). */
int cnerf_field_store16(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const cnerf_volumes* vols, const float* packed,
                        const float* freq, const float* phase, const float* cam2world, const float* u_strat, const float* fine_z, void* feat,
                        void* h, void* c, float* rgb_sigma, void* stream);

/* Stage entry of the storing forward of the per-point FiLM family (csrc/field_pw16.hip: field_pw16_kernel<NT, STORE = true>, then
 * pw_deriv_kernel<NT>), the counterpart of cnerf_field_store16 and what tests/test_gpu_store_pw16.py holds to float64 row by row (added
 * in ABI v10 without a version change: no struct changed).  On the caller's buffers it runs the ONE launch pair cnerf_render_backward
 * runs per pass and chunk when the forward kept no activations.  pass / image0 / n_images / vols / cam2world / u_strat / fine_z as for
 * cnerf_field_store16 (the FULL tensors of the call; pass 2: u_strat carries the points); packed: cnerf_pack_field in
 * CNERF_PREC_FP16X3.  tiles = n_images * ceil(R*R*S / 32), L = cfg->L, NT = H / 32.  Outputs, 16-byte aligned, the chunk's first image
 * first (tile T = image of the chunk * ceil(R*R*S / 32) + tile of the image):
 *   feat            TB16 (tiles, 2, 32, 32) fp16: tile 0 the looked-up feature, fp16(clamp(x, +-65504)); tile 1 the position, rounded to
 *                   nearest, in columns 0..2 and zeros in 3..31.
 *   h               L TB16 slabs (tiles, NT, 32, 32) fp16: y_l = sin(arg_l); then TB16 (tiles, 8, 32, 32): m = LeakyReLU_0.2(Wm1 feat +
 *                   bm1), clamped to +-65504.
 *   c               3 L COS16 slabs (tiles, NT, 4, 64, 4) fp16, the layout of cnerf_field_chain_pw16's cos16: per layer cos(arg_l),
 *                   cos(arg_l) f_l, cos(arg_l) 15 pre_l (f_l = 15 fr_l + 30), the latter two clamped to +-65504.  They are formed by
 *                   pw_deriv_kernel from the STORED cos, m and y_{l-1} (layer 0: the fp16 position) with the leading fp16 part of each
 *                   scaled weight (rounded to nearest: relative 2^-11 per weight).
 *   amax            (L, tiles * 32) fp32: max(1, largest |stored cos f|, |stored cos 15 pre| of the point and layer before their fp16
 *                   rounding): 1 <= amax, every stored derivative d of the point has |d| <= amax (1 + 2^-11).
 *   rgb_sigma       (n_images * R*R*S, 4) fp32: the head's output, equal to cnerf_field_forward's in CNERF_PREC_FP16X3.
 * Rows past an image's end (the padded lanes of an image's last tile) hold the rows of the image's LAST point in feat, y, m, all 3 L
 * slabs of c and amax: the weight reductions multiply them by zero gradient rows (they must be finite whatever the buffer held), and
 * those of amax enter the layer maximum r_l comes from.  A wave without a tile stores nothing; nothing outside the chunk's tiles is written.
 * CNERF_EINVAL and no launch: another layer family, cfg->precision != CNERF_PREC_FP16X3, drop_p != 0, a volume other than one 32-channel
 * level, pass outside 0..2, an image range outside [0, B), a NULL required argument (vols or its level, packed, cam2world of a ray
 * pass, fine_z of the fine pass, the points of pass 2, an output). */
int cnerf_field_store_pw16(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const cnerf_volumes* vols, const float* packed,
                           const float* cam2world, const float* u_strat, const float* fine_z, void* feat, void* h, void* c, float* amax,
                           float* rgb_sigma, void* stream);

/* Stage entry of the half-precision gradient chain of the per-point FiLM family (csrc/chain_pw16.hip: chain_pre_kernel, pw_gm_kernel),
 * the counterpart of cnerf_field_chain16 and what tests/test_gpu_chain_pw16.py holds to float64 row by row (added in ABI v10 without a
 * version change: no struct changed).  On the caller's buffers it runs the launches cnerf_render_backward runs per pass and chunk between
 * the storing forward and the reductions: the head's scale, chain_pre's dry run over the sampled tile groups, the g_y scales, the largest
 * stored derivative per layer (r_l, To_l, the three slab scales), chain_pre, pw_gm's dry run, g_mpre's scale, pw_gm.  pass / image0 /
 * n_images / cam2world / u_strat / fine_z / grad_rgb_sigma / saved_rgb_sigma as for cnerf_field_chain16; tiles = n_images * ceil(R*R*S / 32),
 * L = cfg->L, NT = H / 32.
 *   packed16   cnerf_pack_field_chain16 of the per-point FiLM network.
 *   cos16      3 L COS16 slabs (the layout of cnerf_field_chain16's cos16) of the chunk's tiles: per layer cos, cos f, cos 15 pre.
 *   amax       (L, tiles * 32) fp32: per point and layer the largest |stored derivative| of the three rows (it bounds the operand scale T of
 *              the point and, through its maximum over ALL tiles * 32 entries of a layer, r_l).
 *   m16        TB16 (tiles, 8, 32, 32): the mapping network's hidden activation LeakyReLU_0.2(Wm1 feat + bm1); only its sign is read.
 *   Rows past an image's end (padded lanes of a last tile) of cos16 / m16 may hold any finite values: they reach no output.  Those of amax
 *   enter the layer maximum r_l comes from: finite, >= 0 and below 3e38 (a larger value reads as "no maximum": r_l = 1); the storing
 *   forward writes the image's last point there.
 *   group_step 0: the render's rule (every (groups / 1024)-th group of four tiles, 1..32); k >= 1: both dry runs sample every k-th.
 * Outputs (rows past an image's end are 0 in every TB16 slab):
 *   gy16       TB16 (L, tiles, NT, 32, 32): d loss / d y_l times S_y,l = scales[2 (3 L + 2 + l)].
 *   g16        TB16 (3 L, tiles, NT, 32, 32): per layer g_pre = g_y cos f, g_fr = g_y cos 15 pre, g_ph = g_y cos, each exactly
 *              fp16(gy16 * derivative * r_l), i.e. times scales[2 (3 l + s)] = S_y,l r_l; then g_mpre TB16 (tiles, 8, 32, 32) times scales[2 (3 L)].
 *   go16       TB16 (tiles, 1, 32, 32): d loss / d (head pre-activation) times scales[2 (3 L + 1)] in channels 0..3, zeros elsewhere.
 *   scales     2 (4 L + 2) + 2 L floats: {S, 1 / S} for slots 3 l + s (s = 0 g_pre, 1 g_fr, 2 g_ph), 3 L (g_mpre), 3 L + 1 (go), 3 L + 2 + l
 *              (g_y of layer l); then `lay`: {r_l, To_l = 8 r_l} per layer, r_l = 2^-ceil(log2 max(1, largest amax of layer l)).
 *   gmax       5 L + 2 words, the bits of non-negative floats: slots 0 .. 3 L - 1 unused (0), 3 L: largest sampled |g_mpre|, 3 L + 1: largest
 *              sampled head gradient, 3 L + 2 + l: largest sampled |g_y_l|, 4 L + 2 + l: largest amax of layer l; the head's scale comes
 *              from the largest |grad_rgb_sigma| of the chunk, which passes through slot 3 L + 1 before the dry run overwrites it.
 *   grad_vols  the FULL gradient volume, ACCUMULATED INTO by pw_gm's own atomics (g_feat = Wm1^T g_mpre, trilinear weights).
 *   saturated  optional: += 1 per (tile, layer) with a point whose stored g_y was clamped to fp16's range or whose operands of the mapping
 *              products fp16(gy16 * derivative * To_l) can pass it ((max |g_y| S_y,l) * amax * To_l > 65472: such operands are +-inf, the
 *              point's g_mpre and the voxels it reaches may hold NaN), and per tile whose g_mpre was clamped: non-zero means repeat in
 *              fp32, as in cnerf_render_backward.
 * CNERF_EINVAL and no launch: another layer family, a volume other than one 32-channel level, cfg->precision != CNERF_PREC_FP16X3, pass
 * outside 0..2, an image range outside [0, B), group_step < 0, a NULL required argument (cam2world of a ray pass, fine_z of the fine pass,
 * the points of pass 2, grad_vols and its level among them). */
int cnerf_field_chain_pw16(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const void* packed16, const float* cam2world,
                           const float* u_strat, const float* fine_z, const float* grad_rgb_sigma, const float* saved_rgb_sigma, const void* cos16,
                           const float* amax, const void* m16, int32_t group_step, void* gy16, void* g16, void* go16, float* scales, uint32_t* gmax,
                           const cnerf_grad_volumes* grad_vols, uint32_t* saturated, void* stream);
int cnerf_render_backward(const cnerf_cfg* cfg, int32_t backward_precision, int32_t images_per_chunk, const cnerf_volumes* vols,
                          const cnerf_field_params* params, const float* packed, const void* packed_bwd, const float* freq,
                          const float* phase, const float* cam2world, const cnerf_rng* rng, const cnerf_saved* saved,
                          const cnerf_aux* act16, const float* grad_pixels, const float* grad_depth,
                          const cnerf_field_param_grads* grads, float* grad_freq, float* grad_phase,
                          const cnerf_grad_volumes* grad_vols, uint32_t* saturated, void* workspace, void* stream);

/* ---- gradients of a field query (ABI v9): autograd twin of cnerf_field_forward --------------------------------------------
 * Replaces loss.backward() through <SIREN>.forward(points, z, img_size, num_steps) (siren.py:628-670 under autograd): the inputs are
 * the forward's (cfg, vols, freq / phase, points (B,n,3), n_per_image), its output rgb_sigma (saved_rgb_sigma, (B,n,4)) and
 * d loss / d rgb_sigma (grad_rgb_sigma, (B,n,4)).  Per image and range of points_per_chunk points it runs the render's chunk body of
 * that backward precision -- the activation-storing re-run of the forward, the gradient chain (whose feature-volume gradients go to
 * grad_vols with the chain's own atomics: points are no pixel patches), one weight reduction per matrix -- and, when grad_points is
 * given, the position gradient (csrc/points_grad.hip): layer 0's input gradient from the chunk's layer-0 gradient slab, its lookup
 * term through the trilinear weights of every level (ATen grid_sampler_3d_backward, border padding: zero on an axis whose coordinate
 * sits at or beyond the clamp) plus the xyz columns of TALLSIREN_dgx / TALLSIREN's layer 0.
 *   backward_precision  as cnerf_render_backward, with the same coverage: CNERF_PREC_FP32 re-runs the forward in cfg->precision,
 *                       CNERF_PREC_FP16 needs cfg->precision = CNERF_PREC_FP16X3; per-point FiLM + CNERF_PREC_FP32 needs cfg->precision =
 *                       CNERF_PREC_FP32 (per chunk what the stage calls spell: cnerf_field_backward_points, cnerf_pfilm_backward_finish; the
 *                       position gradient: g_pre_0 W_0 plus the lookup term of the stage's d feat rows).
 *   packed / packed_bwd as cnerf_render_backward.  cfg->R, S, fov are not read (check as for cnerf_field_forward).
 *   grads, grad_freq, grad_phase, grad_vols, grad_points (B,n,3) or NULL = skip: ACCUMULATED INTO (zero them first).
 *   dropout (cfg->drop_p > 0, fp32 only): the decisions of cnerf_field_forward (stream 6 at the point's index in the whole call),
 *                       whatever the chunking.
 *   saturated           as cnerf_render_backward (fp16 backward).
 *   workspace           cnerf_field_query_backward_workspace_bytes(cfg, backward_precision, points_per_chunk): grows with
 *                       points_per_chunk, independent of n. */
int cnerf_field_query_backward_workspace_bytes(const cnerf_cfg* cfg, int32_t backward_precision, int64_t points_per_chunk, size_t* bytes);
int cnerf_field_query_backward(const cnerf_cfg* cfg, int32_t backward_precision, int64_t points_per_chunk, const cnerf_volumes* vols,
                               const cnerf_field_params* params, const float* packed, const void* packed_bwd, const float* freq,
                               const float* phase, const float* points, int64_t n_per_image, const float* saved_rgb_sigma,
                               const float* grad_rgb_sigma, const cnerf_field_param_grads* grads, float* grad_freq, float* grad_phase,
                               const cnerf_grad_volumes* grad_vols, float* grad_points, uint32_t* saturated, void* workspace, void* stream);

/* Stage entries of the per-point FiLM family's exact fp32 query backward (followed per chunk by cnerf_pfilm_backward_finish, as
 * cnerf_field_backward is for the ray passes), for hosts that sequence the stages themselves -- cnerf_field_query_backward runs them all:
 *   cnerf_field_backward_points  cnerf_field_backward (pass 2) for ANY point count: points / grad_rgb_sigma / saved_rgb_sigma are
 *                                (B, n_per_image, ...) of cfg->B images (cfg->R, S unused); act_* sized for B * n_per_image rows;
 *                                drop_mask (n_drop, B * n_per_image, H) or NULL (then Philox stream 6 at index b * n_per_image + p).
 *   cnerf_feature_points_grad    position-side counterpart of cnerf_scatter_features: grad_points (B,n,3) += sum over levels and
 *                                channels of grad_feat (B,n,C) * d feat / d points (lookup term, border rule as above).
 *   cnerf_dropout_keep           keep bytes (n_drop, n_points, H) of points [point0, point0 + n_points) of a call: the decisions the
 *                                kernels draw on Philox stream stream_id (4..6) under cfg's key, drop_p and layers. */
int cnerf_field_backward_points(const cnerf_cfg* cfg, const cnerf_volumes* vols, const float* packed, const float* packed_t, const float* freq,
                                const float* phase, const float* points, int64_t n_per_image, const float* grad_rgb_sigma,
                                const float* saved_rgb_sigma, float* act_feat, float* act_h, float* act_c, float* act_g, float* act_go,
                                const cnerf_grad_volumes* grad_vols, const uint8_t* drop_mask, void* stream);
int cnerf_feature_points_grad(const cnerf_cfg* cfg, const cnerf_volumes* vols, const float* points, int64_t n_per_image, const float* grad_feat,
                              float* grad_points, void* stream);
int cnerf_dropout_keep(const cnerf_cfg* cfg, uint32_t stream_id, int64_t point0, int64_t n_points, uint8_t* mask, void* stream);

/* Everything of the per-point FiLM family's exact fp32 backward that follows cnerf_field_backward / cnerf_field_backward_points on
 * one chunk (n = n_images * n_per_image rows): the parameter gradients of the L layers, the head and the mapping network, d feat and
 * its scatter.  Autograd of the mapping network and the nn.Linear layers of TALLSIREN (siren.py:81-101, 232-331) for hosts without a
 * GEMM library; added in ABI v10 without a version change (no struct changed).  cnerf_render_backward and cnerf_field_query_backward
 * run this stage per chunk themselves; the entry stays for hosts that sequence the stages.
 * cfg: PFILM network, precision FP32, one 32-channel volume (else CNERF_EINVAL; cfg->B, R, S are not read).  Chunk inputs exactly as
 * cnerf_field_backward left them:
 *   points (n,3)  act_feat (n,32)  act_h: L slabs y_l (n,H) then m (n,256)  act_g: L slabs g_pre_l (n,H) then G (n,2LH)  act_go (n,4)
 * Outputs, all ACCUMULATED INTO with float atomics (NULL = skip):
 *   grads->w[l], b[l] (layer 0: (H,3) against points), w_final, b_final, map_w1, map_b1, map_w2, map_b2
 *   grad_fvol_cl (n_images,V,V,V,32): scatter of d feat = g_mpre Wm1 with the trilinear weights of points (image = row / n_per_image)
 *   grad_feat (n,32) or NULL: d feat itself, OVERWRITTEN -- the very rows the scatter read (the query path feeds them to
 *                    cnerf_feature_points_grad)
 * params is not read (both mapping matrices come from packed_map) and may be NULL.  packed_map: written by
 * cnerf_pack_pfilm_map_transposed from params->map_w1 / map_w2, a buffer of its own -- cnerf_backward_bytes /
 * cnerf_pack_field_transposed keep their contents for this family.  workspace: cnerf_pfilm_finish_bytes(cfg, n_images, n_per_image);
 * it begins with g_mpre (n,256) = (G Wm2) * (m > 0 ? 1 : 0.2), which stays readable after the call.  packed_map, act_*, grad_feat and
 * workspace must be 16-byte aligned.  Nothing is allocated or synchronised; a bad argument returns CNERF_EINVAL and launches nothing. */
int cnerf_pfilm_finish_bytes(const cnerf_cfg* cfg, int32_t n_images, int64_t n_per_image, size_t* packed_map, size_t* workspace);
int cnerf_pack_pfilm_map_transposed(const cnerf_cfg* cfg, const cnerf_field_params* params, void* packed_map, void* stream);
int cnerf_pfilm_backward_finish(const cnerf_cfg* cfg, const cnerf_field_params* params, const void* packed_map,
                                int32_t n_images, int64_t n_per_image, const float* points, const float* act_feat,
                                const float* act_h, const float* act_g, const float* act_go,
                                const cnerf_field_param_grads* grads, float* grad_fvol_cl, float* grad_feat,
                                void* workspace, void* stream);

/* ---- ray batches: the render on caller-given rays (added in ABI v10 without a version change: no struct changed) ------------------
 * cnerf_render_forward serves one camera model, the square R x R pinhole grid derived from (cam2world, fov).  These entries take
 * the rays themselves -- P = rays_per_image world origins and directions per image, any P >= 1 -- so a caller can render a crop or a
 * non-square image, a random subset of pixels, intrinsics with a principal-point offset, a large image in tiles, and can
 * differentiate with respect to the rays (camera).  Replaces ImplicitGenerator3d.forward (generators.py:33-187) from line 95 on, for
 * rays formed by the caller instead of get_initial_rays_trig / transform_sampled_points (volumetric_rendering.py:73-199).
 *
 *   cfg        R and fov_deg are not read; S in [2,128]; the rest as cnerf_field_forward checks it.  The flags HIERARCHICAL, WHITE_BACK,
 *              LAST_BACK, SOFTPLUS, noise_std, philox* and ray_start / ray_end keep their meaning.  drop_p > 0: CNERF_EINVAL (the grid
 *              render has dropout).  Every layer family and precision of cnerf_field_forward / cnerf_field_query_backward.
 *   rng        cnerf_rng with P in place of R*R; Philox streams 0-3 are indexed by (b P + p) S + s.  fine_z teacher-forces the fine pass.
 *              drop_coarse / drop_fine are not read.
 *   aux        cnerf_aux intermediates with P in place of R*R (sort_idx, final_weights per ray); act16 and field_events are ignored.
 *
 * Arithmetic: coarse depth z = zl[s] + (u - 0.5) (zl[1] - zl[0]) with zl = torch.linspace(ray_start, ray_end, S) -- bit-identical to the
 * grid render's coarse_z for the same u (u_strat, else Philox, else 0.5); sample position per component p = o + d z, the product
 * rounded, then the sum (no fma), in both passes: generators.py:138-142.  Depths are in units of |dir|: directions are not normalised
 * here.  The field runs at those explicit points (the kernels of cnerf_field_forward, unfolded FiLM); resampling, the merge by depth and
 * the compositing are the grid render's kernels.  Outputs per ray: pixels (B,P,3) = 2 rgb - 1 and dist (B,P) = sum w z, the distance
 * along the ray in units of |dir| -- depth along a camera axis is the caller's business.
 *
 * Backward: cnerf_merge_composite_backward's kernel on per-ray gradients, then per pass (coarse, fine) the sample positions again from
 * the saved depths and what cnerf_field_query_backward runs on them, chunked by points_per_chunk (the feature-volume gradient by the
 * chain's own atomics; no patch scatter).  Sample depths carry no gradient (generators.py:57,111), so with g_s the position gradient of
 * sample s:  grad_origins[b,p] += sum_s g_s,  grad_dirs[b,p] += sum_s z_s g_s  over the coarse, then the fine samples, reduced by one
 * wave per ray in a fixed order without atomics: two runs agree bit for bit.  All gradient buffers are ACCUMULATED INTO (zero them
 * first); grad_dist, grad_origins, grad_dirs may be NULL.  backward_precision, params, packed, packed_bwd, grads, saturated: as
 * cnerf_field_query_backward; saved: the forward's cnerf_aux tensors (fine_z: the depths the fine pass used, i.e. rng->fine_z when forced).
 * Every refusal happens before any launch; nothing is allocated or synchronised. */
typedef struct cnerf_rays {          /* HOST struct of device pointers */
    const float* origins;            /* (B,P,3) world */
    const float* dirs;               /* (B,P,3) world; depths are in units of |dir| (not normalised here) */
} cnerf_rays;

int cnerf_render_rays_workspace_bytes(const cnerf_cfg* cfg, int64_t rays_per_image, size_t* fwd_ws);
int cnerf_render_rays_forward(const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_volumes* vols,
                              const float* packed, const float* freq, const float* phase, const cnerf_rng* rng,
                              float* pixels /* (B,P,3) = 2*rgb-1 */, float* dist /* (B,P) = sum w z */, const cnerf_aux* aux,
                              void* workspace, void* stream);
int cnerf_render_rays_backward_workspace_bytes(const cnerf_cfg* cfg, int32_t backward_precision, int64_t rays_per_image,
                                               int64_t points_per_chunk, size_t* bytes);
int cnerf_render_rays_backward(const cnerf_cfg* cfg, int32_t backward_precision, int64_t points_per_chunk, const cnerf_rays* rays,
                               int64_t rays_per_image, const cnerf_volumes* vols, const cnerf_field_params* params, const float* packed,
                               const void* packed_bwd, const float* freq, const float* phase, const cnerf_rng* rng,
                               const cnerf_saved* saved, const float* grad_pixels /* (B,P,3) */, const float* grad_dist /* (B,P) or NULL */,
                               const cnerf_field_param_grads* grads, float* grad_freq, float* grad_phase,
                               const cnerf_grad_volumes* grad_vols, float* grad_origins /* (B,P,3) or NULL */,
                               float* grad_dirs /* (B,P,3) or NULL */, uint32_t* saturated, void* workspace, void* stream);

/* ---- occupancy grids: forward-only ray renders that skip empty space (added in ABI v10 without a version change: no struct changed) ----
 * An inference job renders one conditioned scene from many cameras (the reference's render_video, render_pcl and
 * _inference_fixed_camera loops), and most samples of a ray fall where the field has no density.  An occupancy grid marks the cells of a
 * cube that can hold density; a sample in a cell that cannot is not given to the field network.  The reference has no such stage.
 *
 * A grid belongs to ONE image of the call: G^3 bits (G a multiple of 4 in [4,256]) over the axis-aligned cube with corner lo[3] and edge
 * `side`; bit index (ix G + iy) G + iz in word idx >> 5, bit idx & 31, where (x, y, z) are columns 0, 1, 2 of a point.  Cell coordinate
 * per axis, in fp32 with every operation rounded on its own:  inv = (float)G / side (once, on the host), t = (p - lo) * inv; the point is
 * INSIDE iff 0 <= t < G on all three axes (a NaN is not inside), and then its cell is floor(t).  A point is LIVE iff it is not inside or
 * its cell's bit is set: outside the cube nothing is skipped, so choose a cube that covers the rays.  A point that is not live is not
 * evaluated; its rgb_sigma is (0, 0, 0, -inf), which both clamp modes turn into density 0 (with noise_std != 0 as well: -inf + noise is
 * -inf).  Live points go through the kernels of cnerf_field_forward and get bit for bit the values of an unmasked call at the same precision.
 *
 *   cnerf_occupancy_build    sigma (B, (G+1)^3): the density at the cell corners, index (ix (G+1) + iy) (G+1) + iz.  m of a cell = maximum
 *                            over its 8 corners; m' = maximum of m over the cells within `dilate` (0..4) of it on every axis, clipped at the
 *                            grid; the bit is set iff !(m' <= threshold).  The maxima keep a NaN, so a NaN corner sets its bits.
 *                            bits (B, G^3 / 32), 8-byte aligned, every word written.
 *   cnerf_occupancy_compact  points (B,n,3), n < 2^31 -> rank (B,n) int32: the point's index among its image's live points in ascending
 *                            order, -1 if it is skipped; live_points (B,n,3): image b's live positions packed at the front of its n rows
 *                            (the rows behind counts[b] are not written); counts (B) DEVICE int32.  Stable and deterministic: ballots and
 *                            scans, no atomics.  workspace: cnerf_occupancy_compact_bytes.
 *   cnerf_occupancy_expand   rgb_sigma[b,i] = rank[b,i] >= 0 ? live_rgb_sigma[b, rank[b,i]] : (0, 0, 0, -inf); both (B,n,4), 16-byte aligned,
 *                            distinct buffers.
 * All three are asynchronous on `stream` and allocate nothing.
 *
 *   cnerf_render_rays_masked_forward   cnerf_render_rays_forward with each field pass replaced by: compact, copy the B counts to the host
 *                            and SYNCHRONISE THE STREAM (so: twice per hierarchical call, once otherwise -- unlike every other entry this one
 *                            blocks the calling thread, and it refuses a stream that is being captured), one field launch per image on
 *                            counts[b] points (none when the count is 0), expand.  Resampling, merge and compositing run as they are.
 *                            occ->bits holds one grid per image of the call.  aux pointers mean what they mean in cnerf_render_rays_forward
 *                            (coarse / fine rgb_sigma: the expanded tensors).  live_counts: HOST int32 (2,B) or NULL -- row 0 the coarse,
 *                            row 1 the fine pass (row 1 is not written when not hierarchical).  No backward, no dropout.
 *                            CNERF_EINVAL before any launch: what cnerf_render_rays_forward refuses (drop_p > 0 among it), occ NULL, G not
 *                            a multiple of 4 in [4,256], side <= 0, bits NULL, a capturing stream.
 *                            workspace: cnerf_render_rays_masked_workspace_bytes. */
typedef struct cnerf_occupancy {     /* HOST struct */
    const uint32_t* bits;            /* (B, G*G*G/32) device */
    int32_t G;
    float lo[3];
    float side;
} cnerf_occupancy;

int cnerf_occupancy_build(int32_t B, int32_t G, int32_t dilate, float threshold, const float* sigma, uint32_t* bits, void* stream);
int cnerf_occupancy_compact_bytes(int32_t B, int64_t n_per_image, size_t* workspace);
int cnerf_occupancy_compact(const cnerf_occupancy* occ, int32_t B, int64_t n_per_image, const float* points, int32_t* rank,
                            float* live_points, int32_t* counts /* (B) device */, void* workspace, void* stream);
int cnerf_occupancy_expand(int32_t B, int64_t n_per_image, const int32_t* rank, const float* live_rgb_sigma, float* rgb_sigma, void* stream);
int cnerf_render_rays_masked_workspace_bytes(const cnerf_cfg* cfg, int64_t rays_per_image, size_t* bytes);
int cnerf_render_rays_masked_forward(const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_occupancy* occ,
                                     const cnerf_volumes* vols, const float* packed, const float* freq, const float* phase,
                                     const cnerf_rng* rng, float* pixels /* (B,P,3) */, float* dist /* (B,P) */, const cnerf_aux* aux,
                                     int32_t* live_counts /* HOST int32 (2,B) or NULL */, void* workspace, void* stream);

/* ---- per-ray sampling bounds (added in ABI v10 without a version change: no struct changed, additive symbols only) -------------------
 * cnerf_render_rays_forward places the S coarse samples of every ray over the one interval [cfg.ray_start, cfg.ray_end].  The entries
 * below place them over an interval of the ray's own, and cnerf_occupancy_ray_bounds takes such intervals from an occupancy grid: the
 * span of the ray that crosses set cells.  The reference has neither.
 *
 *   cnerf_render_rays_bounded_forward, cnerf_render_rays_bounded_masked_forward
 *       cnerf_render_rays_forward / cnerf_render_rays_masked_forward (which are these two with bounds == NULL) with the coarse depths
 *       z = zl[s] + (u - 0.5) (zl[1] - zl[0]),  zl = torch.linspace(near[b,p], far[b,p], S):  the same linspace, order of roundings and
 *       Philox indexing, so near / far filled with ray_start / ray_end give the unbounded call's bits.  The fine pass, the merge and the
 *       compositing do not change.  bounds NULL, or both members NULL: the scalars of cfg.  CNERF_EINVAL before any launch: what the
 *       unbounded entry refuses; only one of near / far given.  The values are not checked: far <= near, a NaN or an infinity give the
 *       depths that arithmetic gives.  Workspaces: those of the unbounded entries.
 *       There is no bounded backward entry and none is needed: the depths carry no gradient (generators.py:57,111), and
 *       cnerf_render_rays_backward re-forms the sample positions from saved->coarse_z / fine_z, never from ray_start / ray_end -- pass
 *       it the tensors a bounded forward saved.
 *
 *   cnerf_occupancy_ray_bounds   near, far (B,P) float32 and hit (B,P) uint8 (may be NULL) of rays (B,P), one grid per image.
 *       Contract, exact on the real line (the fp32 kernel's error is stated below).  Omega_b = the union of the CLOSED cells of image b
 *       whose bit is set, cell (ix, iy, iz) = the product of [lo_k + i_k side / G, lo_k + (i_k + 1) side / G];  T = the set of t in
 *       [t_min, t_max] with o + t d in Omega_b.
 *         T empty:    hit = 0, near = t_min, far = t_max -- a missed ray is sampled as it always was, never over a degenerate interval.
 *         otherwise:  hit = 1, near = max(t_min, inf T - pad), far = min(t_max, sup T + pad); if that leaves far <= near the ray counts
 *                     as missed (so with pad = 0 a ray that only touches Omega_b at one depth is a miss).
 *       t and pad are in units of |dir|, like every depth of the ray path: for a pad of a length in space divide it by |dir|.
 *       Segments of a ray OUTSIDE the cube count as EMPTY here -- unlike the liveness rule of the masked render above, where nothing
 *       outside the cube is skipped.  Samples placed over [near, far] therefore see nothing of density outside the cube.
 *       The kernel clips the ray to the cube (slab test) and walks the cells it crosses over the whole clipped span (3-D DDA over the bit
 *       words, at most 3 G + 3 steps, one lane per ray, no atomics: deterministic).  fp32, every operation rounded on its own: plane j of
 *       axis k at lo_k + (float)j * (side / (float)G), crossed at (plane - o_k) / d_k, each depth formed from its plane index, none
 *       accumulated.  With M the largest coordinate magnitude among the origin and the cube's corners, [near, far] of a hit lies
 *       between the exact hulls for every set cell shrunk and grown by 32 * 2^-23 * M in space, and hit is exact outside that margin.
 *       A component d_k == 0 (either sign) is not divided by: the ray misses unless o_k is in the cube's slab.  A NaN or an infinity in
 *       the ray's origin or direction: a miss.  A ray that starts inside the cube starts at t_min; t_min beyond the exit: a miss.
 *       CNERF_EINVAL before the launch: the grid checks of cnerf_occupancy_compact, rays / near / far NULL, B or rays_per_image < 1,
 *       t_min or t_max not finite, t_max <= t_min, pad < 0 or not finite.  Asynchronous on `stream`, allocates nothing. */
typedef struct cnerf_ray_bounds {    /* HOST struct of device pointers */
    const float* near;               /* (B,P) */
    const float* far;                /* (B,P) */
} cnerf_ray_bounds;

int cnerf_occupancy_ray_bounds(const cnerf_occupancy* occ, const cnerf_rays* rays, int32_t B, int64_t rays_per_image, float t_min, float t_max,
                               float pad, float* near /* (B,P) */, float* far /* (B,P) */, uint8_t* hit /* (B,P) or NULL */, void* stream);
int cnerf_render_rays_bounded_forward(const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_ray_bounds* bounds,
                                      const cnerf_volumes* vols, const float* packed, const float* freq, const float* phase, const cnerf_rng* rng,
                                      float* pixels /* (B,P,3) */, float* dist /* (B,P) */, const cnerf_aux* aux, void* workspace, void* stream);
int cnerf_render_rays_bounded_masked_forward(const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_ray_bounds* bounds,
                                             const cnerf_occupancy* occ, const cnerf_volumes* vols, const float* packed, const float* freq,
                                             const float* phase, const cnerf_rng* rng, float* pixels /* (B,P,3) */, float* dist /* (B,P) */,
                                             const cnerf_aux* aux, int32_t* live_counts /* HOST int32 (2,B) or NULL */, void* workspace,
                                             void* stream);

/* ---- isosurfaces: an indexed triangle mesh of a scalar lattice (added in ABI v10 without a version change: additive symbols only) -----
 * The other consumer of a conditioned field is its shape (the reference's extract_shapes.py samples sigma on an N^3 grid and leaves the
 * surface to outside tools).  These entries turn a scalar lattice on the device into vertices and triangles on the device, by marching
 * tetrahedra on the Kuhn split of every cell.  The algorithm is fixed here so that it can be checked exactly.
 *
 * Lattice.  values v[i0,i1,i2], (n0,n1,n2) row-major fp32, each n_c in [2,1024], n0 n1 n2 <= 2^27 (both totals then fit int32).  Point
 *   (i0,i1,i2) sits at position component c = (float)i_c * pitch + lo[c]: the product rounded, then the sum, no fma.
 * Cells.  A point is INSIDE iff v > level: a value equal to the level is outside, a NaN is outside.  Cell (i0,i1,i2) exists for
 *   i_c < n_c - 1 and is cut into the six tetrahedra of the Kuhn triangulation: tetrahedron t belongs to the axis permutation (a,b,c),
 *   in lexicographic order 012, 021, 102, 120, 201, 210, with vertices w0 = corner, w1 = w0 + e_a, w2 = w1 + e_b, w3 = corner + (1,1,1).
 *   Every tetrahedron edge points in a non-negative direction and is OWNED by its lower endpoint; it has one of seven kinds
 *   k = d0 + 2 d1 + 4 d2 - 1 for the offset (d0,d1,d2) in {0,1}^3 \ 0: three axis edges, three face diagonals, the body diagonal.  The
 *   split is translation invariant, so neighbouring cells agree on every shared face diagonal: the mesh is watertight by construction and
 *   there are no ambiguous cases, at 2-3 times the triangles of marching cubes.
 * Vertices.  One per lattice edge (both ends in the lattice) whose ends differ in INSIDE, numbered by (owner's flat index
 *   (i0 n1 + i1) n2 + i2 ascending, kind ascending).  Position in fp32, every operation rounded on its own, always from the owner P0 to
 *   the other end P1:  t = (level - v0) / (v1 - v0),  pos_c = P0_c + t * (P1_c - P0_c);  t = 0.5 if either end's value is not finite.
 *   attrs (n0,n1,n2,C), 1 <= C <= 8, are interpolated with the same t: a0 + t * (a1 - a0).
 * Triangles.  Ordered by (cell flat index (i0 (n1-1) + i1) (n2-1) + i2 ascending, tetrahedron 0..5, triangle 0..1), each a triple of
 *   vertex indices.  E(x,y) = the vertex on edge w_x w_y.  One vertex m alone on its side, the others p < q < r: (E(m,p), E(m,q), E(m,r)).
 *   Two inside a < b, two outside c < d: the quad q0..q3 = E(a,c), E(a,d), E(b,d), E(b,c) as (q0,q1,q2) and (q0,q2,q3).  The last two
 *   indices of a triangle are exchanged where needed so that its right-hand normal points from INSIDE to outside, toward falling values;
 *   whether depends on (tetrahedron parity, 4-bit case) only.  Zero-area triangles occur where an outside corner equals the level; they
 *   are kept, so the index structure stays closed.
 *
 *   cnerf_isosurface_bytes   workspace of a lattice: 9 bytes per point (the 8 INSIDE bits of a point and its forward neighbours, its
 *                            vertex offset, its cell's triangle offset) and two sums per block of 256 points.
 *   cnerf_isosurface_count   classifies every point and scans: counts = DEVICE int32[2] (vertices, triangles), workspace filled for emit.
 *   cnerf_isosurface_emit    writes vertices (max_vertices,3), vertex_attrs (max_vertices,C) and triangles (max_triangles,3) int32 from the
 *                            workspace as count left it (same lattice, values and level).  A row at or beyond a capacity is skipped, never
 *                            written; rows the surface does not reach are left as they are.
 * Both are asynchronous on `stream` and allocate nothing; the caller copies counts to the host between them, which is the only
 * synchronisation.  Ballots, popcounts and one block's scan, no atomics, no block waits for another: two runs agree bit for bit.
 * CNERF_EINVAL before any launch: an n_c outside [2,1024] or n0 n1 n2 > 2^27; values / counts / workspace / lo / vertices / triangles
 * NULL; level, pitch or a lo[c] not finite, pitch <= 0; attrs given with n_attr outside [1,8]; attrs without vertex_attrs or the reverse;
 * a negative capacity. */
int cnerf_isosurface_bytes(int32_t n0, int32_t n1, int32_t n2, size_t* workspace);
int cnerf_isosurface_count(int32_t n0, int32_t n1, int32_t n2, const float* values, float level,
                           int32_t* counts /* DEVICE int32[2]: vertices, triangles */, void* workspace, void* stream);
int cnerf_isosurface_emit(int32_t n0, int32_t n1, int32_t n2, const float* values, float level, const float lo[3], float pitch,
                          const float* attrs /* (n0,n1,n2,C) or NULL */, int32_t n_attr,
                          int64_t max_vertices, int64_t max_triangles,
                          float* vertices /* (max_vertices,3) */, float* vertex_attrs /* (max_vertices,C) or NULL */,
                          int32_t* triangles /* (max_triangles,3) */, const void* workspace /* as count left it */, void* stream);

/* ---- connected components of a scalar lattice (added in ABI v10 without a version change: additive symbols only) -----------------------
 * What a mesh of a raw density or of a fused volume needs next: which lattice points hang together, so that floaters can be dropped
 * and enclosed free space filled before cnerf_isosurface_* runs, without the lattice leaving the device.  Everything here is an integer
 * and fixed by the lattice alone, so it can be checked exactly.
 *
 * Lattice.  values v[i0,i1,i2], (n0,n1,n2) row-major fp32, the limits of cnerf_isosurface_*: each n_c in [2,1024], n0 n1 n2 <= 2^27.
 *   The flat index of a point is (i0 n1 + i1) n2 + i2.
 * Selection.  A point is INSIDE iff v > level, the isosurface's rule: a value equal to the level is outside, a NaN is outside.
 *   invert = 0 selects the INSIDE points, invert = 1 all the others.
 * Neighbours.  connectivity = 14: two selected points are joined iff they differ by +-(d0,d1,d2), (d0,d1,d2) in {0,1}^3 \ 0 -- the
 *   seven edge kinds of the isosurface's Kuhn split, in both directions ((1,-1,0) is not among them).  These are exactly the lattice
 *   edges on which cnerf_isosurface_* places a vertex when the ends differ in INSIDE, so the components are the pieces that the mesh
 *   separates: moving a whole component to the other side of the level removes its sheets and nothing else, and every vertex and
 *   triangle that is left is bit for bit one of the unfiltered mesh.  Marching tetrahedra treats inside and outside alike, so the same
 *   neighbourhood serves invert = 1.  connectivity = 6: the three axis kinds only (the customary neighbourhood; the property above does
 *   not hold for it).
 * Results.
 *   labels (n0,n1,n2) int32   -1 for a point that is not selected, else the smallest flat index among the points of its component
 *                             (the component's root: labels[root] == root)
 *   sizes  (n0,n1,n2) int32   the point count of a component at the position of its root, 0 everywhere else
 *   stats  DEVICE int32[4]    n_components; largest_root (the root of the component with the most points, at equal size the lowest
 *                             root, -1 if there is no component); largest_size; status (0, or non-zero if a loop cap was hit: the
 *                             other results are then not to be used.  A chain of parents cannot be longer than the lattice has points,
 *                             which is the cap of every loop that follows one, so correct code never reaches it.)
 *   All of them are independent of launch geometry and arrival order: two runs agree bit for bit.
 *
 *   cnerf_components_bytes    workspace of cnerf_components_label (the 64-bit key of the largest component; 8-byte aligned).
 *   cnerf_components_label    fills labels, sizes and stats.  labels doubles as the parent array of a union-find in global memory.
 *   cnerf_components_filter   out_values = values, but `fill` where a labelled point's component fails  size >= min_size  or, with
 *                             largest_only = 1,  root == largest_root.  Points with label -1 are copied; with no component at all
 *                             out_values = values.  It reads stats on the device; out_values may be values itself.  The filter does
 *                             not know the level: a caller that wants the failed components on the other side passes such a fill.
 * All are asynchronous on `stream`, allocate nothing, do not synchronise with the host and need no host readback.
 * CNERF_EINVAL before any launch, checked in this order: an n_c outside [2,1024] or n0 n1 n2 > 2^27; values / labels / sizes / stats /
 * workspace / out_values NULL; level not finite; connectivity other than 6 or 14; invert or largest_only outside {0,1}; min_size < 0;
 * fill NaN; (last) a workspace that is not 8-byte aligned. */
int cnerf_components_bytes(int32_t n0, int32_t n1, int32_t n2, size_t* workspace);
int cnerf_components_label(int32_t n0, int32_t n1, int32_t n2, const float* values, float level, int32_t invert, int32_t connectivity,
                           int32_t* labels /* (n0,n1,n2) */, int32_t* sizes /* (n0,n1,n2) */, int32_t* stats /* DEVICE int32[4] */,
                           void* workspace, void* stream);
int cnerf_components_filter(int32_t n0, int32_t n1, int32_t n2, const float* values, const int32_t* labels, const int32_t* sizes,
                            const int32_t* stats, int32_t largest_only, int32_t min_size, float fill,
                            float* out_values /* (n0,n1,n2), may be values */, void* stream);

/* ---- nearest points: the nearest target of every query, between two batched clouds (added in ABI v10 without a version change:
 * additive symbols only) --------------------------------------------------------------------------------------------------------------
 * The primitive under the Chamfer distance and the F-score of a reconstruction (shape_metrics.py).  The search is exact and brute force:
 * every query meets every target of its image, nothing n x m is stored.  The arithmetic and the tie rule are fixed here so that the
 * result can be checked bit for bit.
 *
 * Distance.  Query q, target t, fp32, every operation rounded on its own, no fma:
 *     dx = qx - tx, dy = qy - ty, dz = qz - tz,    d = (dx*dx + dy*dy) + dz*dz.
 * Result.  Per image b: nq = clamp(n_queries[b], 0, n), mt = clamp(n_targets[b], 0, m); a NULL length array stands for n (m).
 *   For query i < nq: idx[b,i] = the SMALLEST j < mt whose d is minimal among the d that are finite, dist2[b,i] = that d.  A d that is
 *   NaN or +inf is never chosen: a NaN or an infinity in either point, or an overflow of the sum.  No target chosen (mt == 0 included):
 *   dist2 = +inf, idx = -1.  Rows i >= nq are written as (+inf, -1) without a search.  Every element of both outputs is written.
 * Reproducibility.  The outputs do not depend on target_splits, on the launch geometry or on the run; there are no atomics.
 * target_splits.  S > 1 cuts the targets [0, mt) of an image into the S ranges [r mt / S, (r+1) mt / S) (integer division), searched by
 *   different blocks; each writes a partial (d, j) per query into the workspace and a second kernel takes the ranges in ascending order
 *   under the same rule.  Empty ranges (S > mt) are harmless.  It pays with few queries and many targets.  0: the library chooses, a pure
 *   function of (B, n, m); cnerf_nearest_points_bytes with the same four numbers reports the workspace that choice needs.
 *
 *   cnerf_nearest_points_tiling   HOST: the search kernel's constants -- queries of a block, targets of a tile (sizes at which a test
 *                                 should look for edges); either pointer may be NULL.
 *   cnerf_nearest_points_bytes    workspace: 0 for one range, else 8 bytes x S x B x n (each half 256-byte aligned).
 *   cnerf_nearest_points          asynchronous on `stream`, allocates nothing.
 * CNERF_EINVAL before any launch: B < 1, n < 1, m < 1, m >= 2^31, B n >= 2^40; queries / targets / dist2 / idx NULL; target_splits
 * outside [0,1024]; workspace NULL when the bytes entry reports more than 0. */
int cnerf_nearest_points_tiling(int32_t* queries_per_block, int32_t* targets_per_tile);
int cnerf_nearest_points_bytes(int32_t B, int64_t n, int64_t m, int32_t target_splits, size_t* workspace);
int cnerf_nearest_points(int32_t B, int64_t n, int64_t m, const float* queries /* (B,n,3) */, const float* targets /* (B,m,3) */,
                         const int32_t* n_queries /* (B) DEVICE or NULL = n */, const int32_t* n_targets /* (B) DEVICE or NULL = m */,
                         int32_t target_splits /* 0 = chosen by the library, else 1..1024 */,
                         float* dist2 /* (B,n) */, int32_t* idx /* (B,n) */, void* workspace, void* stream);

/* ---- voxel grids of coloured point clouds, and their first-hit pictures (added in ABI v10 without a version change: additive symbols
 * only) ---------------------------------------------------------------------------------------------------------------------------
 * Every feature-volume generator is conditioned on a grid (B,4,G,G,G) = [occupancy, r, g, b] that the 3D U-Net encodes.  The reference
 * makes it offline (feature_volume/pcl2voxel.py: open3d's VoxelGrid and a Python loop, one file per resolution) and pictures it with
 * feature_volume/voxel2img.py.  These entries do both on the device, from the cloud the other shape entries already take.
 *
 * Layouts.  layout 0: voxels (B,4,G,G,G) indexed [b, ch, iz, iy, ix] -- what the encoder takes, the reference's .permute(3,2,1,0) --
 *   counts (B,G,G,G) indexed [b, iz, iy, ix].  layout 1: voxels (B,G,G,G,4) indexed [b, ix, iy, iz, ch] -- the order of voxel.npz --
 *   counts [b, ix, iy, iz]; voxels 16-byte aligned.  ch = occupancy, r, g, b; (x, y, z, r, g, b) are columns 0..5 of a point's row.
 * Cube.  Corner lo[3], edge side > 0, G cells per axis, G in [2,256]; inv = (float)G / side, formed once on the host.
 *
 * cnerf_voxelize.  points (B,n,stride) fp32, stride >= 6, n < 2^28; n_points (B) DEVICE int32 clamped to [0,n], NULL = n (as in
 *   cnerf_nearest_points): rows at or beyond it are not read.  fp32, every operation rounded on its own:
 *     - a point with a NaN in x, y or z is skipped;
 *     - clip_margin = m >= 0 (the reference: 1e-4): per axis p' = fminf(fmaxf(p, lo + m), (lo + side) - m), t = (p' - lo) * inv, the
 *       cell is floor(t) clamped into [0, G-1]: no other point is skipped, an infinite coordinate lands in a border cell;
 *     - clip_margin < 0: no clipping, t = (p - lo) * inv, a point with t outside [0, G) on any axis is skipped (an infinity with it),
 *       otherwise the cell is floor(t) -- the rule of cnerf_occupancy_compact;
 *     - colour per channel q = (uint32) rintf(fminf(fmaxf(c, 0), 1) * 16777216.0f), a NaN colour counts as 0.
 *   Per cell the count of its points and the three sums S_c of their q are EXACT integers (64-bit, below 2^52).  Output per cell:
 *   occupancy = count > 0 ? 1 : 0, colour = (float)((double)S_c / ((double)count * 16777216.0)), 0 in an empty cell.  Every element
 *   of voxels is written; counts (may be NULL) gets the count.
 *   Reproducibility.  Integer sums do not depend on the order of addition, so the outputs are the same bits for every launch geometry
 *   and every run, although the sums are formed by atomics.  That is the point of the fixed-point form: a float atomic sum depends on
 *   the order in which the adds arrive.  The quantisation moves a colour by at most 2^-25.
 *   cnerf_voxelize_bytes: the workspace, 32 bytes per cell and image (four 64-bit integers), 16-byte aligned; its contents are scratch.
 *   CNERF_EINVAL before any launch: B < 1, n < 1, n >= 2^28, stride < 6, G outside [2,256], side not finite or <= 0 (or so small
 *   that inv is not finite), a non-finite lo,
 *   a NaN clip_margin, 2 clip_margin >= side, layout outside {0,1}, points / voxels / workspace / lo NULL, a misaligned buffer.
 *
 * cnerf_voxel_first_hit.  The picture of a grid: along each ray the colour of the first occupied cell among S samples, else the
 *   background.  voxels in either layout; rays (B,P,3) origins and dirs, directions not normalised (t in units of |dir|); S in [2,1024].
 *     t_s = element s of torch.linspace(t_min, t_max, S) as ATen computes it in fp32 (the coarse depths of cnerf_render_rays_forward);
 *     p = o + d * t_s per component, the product rounded, then the sum, no fma;  t = (p - lo) * inv per axis;
 *     the sample is INSIDE iff 0 <= t < G on all three axes (a NaN is not inside), its cell is floor(t); it is OCCUPIED iff it is inside
 *     and the cell's occupancy value != 0 (so a NaN occupancy is occupied).
 *   The first occupied sample in ascending s gives pixels = the cell's (r, g, b) as stored -- the grid's own range, NOT 2 rgb - 1 --,
 *   hit_t = t_s, hit_cell = (ix G + iy) G + iz (in both layouts).  None: pixels = background, hit_t = +inf, hit_cell = -1.
 *   A sample outside the cube sees nothing.  The reference's grid_sample(padding_mode="border") smears the border voxels over all of
 *   space; that is NOT reproduced.  Inside the cube, away from the cell faces, floor(t) is the reference's nearest voxel
 *   (mode="nearest", align_corners=False: rint(t - 0.5)).
 *   One lane per ray, no atomics; the outputs depend on nothing but the inputs.  hit_t / hit_cell may be NULL.
 *   CNERF_EINVAL before the launch: the B, G, lo, side, layout checks above; rays_per_image < 1; S outside [2,1024]; t_min or t_max not
 *   finite, t_max <= t_min; rays / origins / dirs / voxels / background / pixels NULL.
 * All are asynchronous on `stream`, allocate nothing and synchronise nothing.  Forward only. */
int cnerf_voxelize_bytes(int32_t B, int32_t G, size_t* workspace);
int cnerf_voxelize(int32_t B, int64_t n, int32_t stride, const float* points /* (B,n,stride) */, const int32_t* n_points /* (B) DEVICE or NULL = n */,
                   int32_t G, const float lo[3], float side, float clip_margin /* >= 0 clips, < 0 does not */, int32_t layout,
                   float* voxels, int32_t* counts /* (B,G,G,G) or NULL */, void* workspace, void* stream);
int cnerf_voxel_first_hit(int32_t B, int64_t rays_per_image, const cnerf_rays* rays, const float* voxels, int32_t G, const float lo[3], float side,
                          int32_t layout, float t_min, float t_max, int32_t S, const float background[3],
                          float* pixels /* (B,P,3) */, float* hit_t /* (B,P) or NULL */, int32_t* hit_cell /* (B,P) or NULL */, void* stream);

/* ---- between depth images and world-space points: back-projection and the z-buffered splat (added in ABI v10 without a version
 * change: additive symbols only) -----------------------------------------------------------------------------------------------
 * cnerf_backproject fuses V rendered depth maps into one coloured cloud (the reference's Inferencer.render_pcl, inference.py:541-559,
 * without its host code); cnerf_splat_points pictures a cloud from cameras with a z-buffer and returns the camera-space depth image
 * that the reference's render_pcl_masked and loss_depth read from files.  Everything is fp32 and every operation is rounded on its own
 * (no fma).  focal = fp32 1 / tan(fov / 2), formed by the caller as the render path forms it (2.187719 at 49.13 degrees; the
 * reference's literal is 2.1875).  A cam2world is 16 floats, row-major 4x4, M[i][j]; its 3x3 block MUST be a rotation (a look-at
 * matrix is): the splat inverts it by transposing.  This is not checked.  R in [2,2048], B V R R < 2^31.
 *
 * cnerf_backproject.  depth (V,R,R); colors NULL or (V,3,R,R) in color_layout 0 -- the generator's pixels -- / (V,R,R,3) in layout 1;
 *   mask NULL or (V,R,R) fp32; cam2world (V,16).  Pixel (v,row,col) with z = depth[v,row,col] is VALID iff z_min < z && z < z_max
 *   (both strict; a NaN is not valid) and, with a mask, mask[v,row,col] > mask_min (the reference: depth_gt > 1e-4).  For a valid pixel
 *     xn = (float)(2 col - (R-1)) / (float)(R-1), yn likewise from row;   xc = (xn / focal) * z, yc = (yn / focal) * z;
 *     world_i = ((M[i][0] xc + M[i][1] yc) + M[i][2] z) + M[i][3], i = 0..2;   colour_c = c * color_scale + color_offset
 *   (the reference un-normalises with 0.5, 0.5).  points (V R R, 6) -- (V R R, 3) without colors -- gets the valid pixels' rows packed
 *   at the front in ascending (v,row,col): ONE cloud over all views, the reference's torch.cat; the rows behind them are not written.
 *   counts (V) int32 on the device: valid pixels per view (their sum is the cloud's length); pixel (V R R) int32: (v R + row) R + col
 *   of every row of the cloud; rank (V,R,R) int32: the pixel's row in the cloud, -1 where it is not valid.  Each of the three may be NULL.
 *   Count, scan, emit with ballots and popcounts over the flat pixel sequence; no atomics: the order is the pixels' own and the outputs
 *   are the same bits for every launch geometry and every run.
 *   cnerf_backproject_bytes: the workspace, one int32 per 256 pixels of every view and one more; its contents are scratch.
 *   CNERF_EINVAL before any launch: V < 1, R outside [2,2048], V R R >= 2^31, focal not finite or <= 0, z_min not finite or < 0, z_max
 *   not finite or <= z_min, a NaN mask_min / color_scale / color_offset, color_layout outside {0,1}, depth / cam2world / points /
 *   workspace NULL.
 *
 * cnerf_splat_points.  points (B,n,stride) fp32, stride >= 3 (x, y, z first; r, g, b are columns 3..5 and need stride >= 6), n < 2^28;
 *   n_points (B) DEVICE int32 clamped to [0,n], NULL = n (as in cnerf_voxelize); cam2world (B,V,16); radius in [0,8].  Per point i and
 *   view, with t = (M[0][3], M[1][3], M[2][3]):
 *     q = p - t;   cam_j = (q0 M[0][j] + q1 M[1][j]) + q2 M[2][j] (the transposed rotation);   z = cam_2;
 *     the point is skipped unless z_min < z && z < z_max (a NaN coordinate fails).  z_min >= 0, so every kept z is a positive finite
 *     float, and the bit patterns of positive floats order like their values;
 *     half = 0.5f * (float)(R-1);   u = ((cam_0 * focal) / z) * half + half, v likewise from cam_1;
 *     the point is skipped unless -(radius+1) < u && u < R + radius and the same for v (float compares: a NaN fails);
 *     col = (int)rintf(u), row = (int)rintf(v);  the point covers the pixels (row + dr, col + dc), |dr|, |dc| <= radius, that lie in the
 *     image, all with the point's own z.
 *   Per pixel the winner is the smallest 64-bit key ((uint64)bits(z) << 32) | (uint32)i: the nearest point, at exactly equal z the
 *   lowest index.  depth (B,V,R,R) = the winner's z, 0 where nothing landed (the reference's "0 = background": loss_depth's gt != 0 and
 *   the mask's > 1e-4 rely on it); index (B,V,R,R) int32 = the winner's i, or -1; pixels (B,V,R,R,3) = the winner's columns 3..5 as
 *   stored, or background[3].  Each of the three may be NULL.
 *   Reproducibility.  The keys are reduced by 64-bit unsigned atomic minima.  A minimum does not depend on the order in which its
 *   operands arrive, so the outputs are the same bits for every launch geometry and every run, although the order of the atomics is
 *   not fixed.  (A float z-buffer without the index in the key would leave ties to the order of arrival.)
 *   cnerf_splat_points_bytes: the workspace, 8 bytes per (b,view,row,col), 8-byte aligned; the entry sets it to all ones itself.
 *   CNERF_EINVAL before any launch: B, V or n < 1, n >= 2^28, R outside [2,2048], B V R R >= 2^31, stride < 3, pixels with stride < 6,
 *   radius outside [0,8], the focal / z_min / z_max checks above, points / cam2world / workspace NULL, background NULL with pixels.
 * All are asynchronous on `stream`, allocate nothing and synchronise nothing.  Forward only. */
int cnerf_backproject_bytes(int32_t V, int32_t R, size_t* workspace);
int cnerf_backproject(int32_t V, int32_t R, const float* depth /* (V,R,R) */, const float* colors /* NULL, (V,3,R,R) or (V,R,R,3) */,
                      int32_t color_layout, const float* mask /* (V,R,R) or NULL */, float mask_min, const float* cam2world /* (V,16) */,
                      float focal, float z_min, float z_max, float color_scale, float color_offset,
                      float* points /* (V R R, 6 or 3) */, int32_t* counts /* (V) DEVICE or NULL */, int32_t* pixel /* (V R R) or NULL */,
                      int32_t* rank /* (V,R,R) or NULL */, void* workspace, void* stream);
int cnerf_splat_points_bytes(int32_t B, int32_t V, int32_t R, size_t* workspace);
int cnerf_splat_points(int32_t B, int64_t n, int32_t stride, const float* points /* (B,n,stride) */, const int32_t* n_points /* (B) DEVICE or NULL = n */,
                       int32_t V, const float* cam2world /* (B,V,16) */, int32_t R, float focal, float z_min, float z_max, int32_t radius,
                       const float background[3], float* depth /* (B,V,R,R) or NULL */, int32_t* index /* (B,V,R,R) or NULL */,
                       float* pixels /* (B,V,R,R,3) or NULL */, void* workspace, void* stream);

/* ---- depth maps fused into a truncated signed distance lattice (added in ABI v10 without a version change: additive symbols only) ----
 * cnerf_tsdf_integrate fuses V rendered depth maps, with their cameras, into a TSDF on a regular lattice.  Its zero level is the surface
 * the views agree on: no density threshold, floaters no view confirms are carved away, colours come from the rendered pixels.
 * Everything is fp32 and every operation is rounded on its own (no fma); positions and camera coordinates are formed per voxel, never
 * stepped.  focal, cam2world (its 3x3 block MUST be a rotation; not checked) and the projection are those of cnerf_splat_points.
 *
 * Lattice (n0,n1,n2), each n_c in [2,1024], n0 n1 n2 <= 2^27.  Point (i0,i1,i2) sits at p_c = (float)i_c * pitch + lo[c]: lattice axis c
 *   is world axis c.  This is the lattice rule of cnerf_isosurface_*, so tsdf (and rgb as attrs) goes straight into it with the same lo
 *   and pitch.  It is NOT extract_mesh's reversed column convention (there the lattice's last axis is world x).
 * Views: depth (V,R,R); colors NULL, (V,3,R,R) in color_layout 0 or (V,R,R,3) in layout 1; cam2world (V,16); V >= 1, R in [2,2048],
 *   V R R < 2^31.
 * Per voxel: sum = 0, n = 0, hidden = 0, csum = 0, cn = 0; then for w = 0 .. V-1 in this order, with t = (M[0][3], M[1][3], M[2][3]):
 *     q = p - t;   cam_j = (q0 M[0][j] + q1 M[1][j]) + q2 M[2][j];   z = cam_2          (the splat's arithmetic)
 *     the view is skipped unless z > 0 (a NaN fails);
 *     half = 0.5f * (float)(R-1);   u = ((cam_0 * focal) / z) * half + half, v likewise from cam_1;
 *     skipped unless -1 < u && u < R && -1 < v && v < R (float compares);   col = (int)rintf(u), row = (int)rintf(v);
 *     skipped unless 0 <= col < R and 0 <= row < R;   d = depth[w,row,col]: the NEAREST pixel, no interpolation;
 *     if z_min < d && d < z_max (a SURFACE pixel):   s = (z - d) / trunc, positive BEHIND the surface;
 *         if s > 1: hidden += 1 (occluded: no observation)
 *         else:     if colors && s >= -1: csum_k = csum_k + (c_k * color_scale + color_offset), k = 0..2; cn += 1
 *                   sum = sum + fmaxf(s, -1); n += 1
 *     else if d is not a NaN (a BACKGROUND pixel: d <= z_min or d >= z_max, +-inf included):   if carve: sum = sum + (-1); n += 1
 *     (a NaN depth says nothing)
 *   tsdf   = n > 0 ? sum / (float)n : (hidden_min > 0 && hidden >= hidden_min ? 1.0f : unseen)
 *   weight = n > 0 ? n : -hidden            (n0,n1,n2) int32 or NULL; 0 = no view says anything about this voxel
 *   rgb_k  = cn > 0 ? csum_k / (float)cn : 0        (n0,n1,n2,3) or NULL; needs colors
 * The sign is inside-positive on purpose: cnerf_isosurface_* at level 0 (INSIDE iff v > 0) then gives normals that point out of the object.
 * The renderer's depth of a ray through empty space is near 0, below ray_start: with z_min = ray_start, z_max = ray_end these are
 *   background pixels.  They carve, and cnerf_backproject discards them likewise.
 * The hidden rule is the visual hull's: a voxel that no view saw free and at least hidden_min views saw behind a surface counts as
 *   solid.  Without it (hidden_min = 0) the deep interior of every closed object is `unseen` and gets a second, inner surface.
 * A voxel outside every image (or behind every camera) takes `unseen`; -1, free, is the usual choice.
 * When only a few cameras cover the cube, hidden_min = 1 can leave small solid blobs in the cube's corners, where a single view sees a
 *   voxel behind the object and none sees it free (measured: 44 of 32,768 voxels with 24 cameras at radius 1.0-1.2 and a cube of side
 *   1.2; none with 48 cameras, or with a cube of side 0.9 seen from radius 1.2-1.6).  Keep the cube inside what the views cover.
 * Reproducibility: each voxel is written by one lane, its views in a fixed order, without atomics: the outputs are the same bits on
 *   every run and for every launch geometry.
 * No workspace; asynchronous on `stream`, allocates nothing and synchronises nothing.  Forward only.
 * CNERF_EINVAL before any launch: an n_c outside [2,1024], n0 n1 n2 > 2^27, V < 1, R outside [2,2048], V R R >= 2^31, pitch / a lo[c] /
 *   unseen / color_scale / color_offset not finite, pitch <= 0, trunc not finite or <= 0, the focal / z_min / z_max checks of
 *   cnerf_backproject, color_layout outside {0,1}, hidden_min < 0, carve outside {0,1}, lo / depth / cam2world / tsdf NULL, rgb without
 *   colors. */
int cnerf_tsdf_integrate(int32_t n0, int32_t n1, int32_t n2, const float lo[3], float pitch, int32_t V, int32_t R,
                         const float* depth /* (V,R,R) */, const float* colors /* NULL, (V,3,R,R) or (V,R,R,3) */, int32_t color_layout,
                         float color_scale, float color_offset, const float* cam2world /* (V,16) */, float focal, float z_min, float z_max,
                         float trunc, int32_t carve, int32_t hidden_min, float unseen, float* tsdf /* (n0,n1,n2) */,
                         int32_t* weight /* (n0,n1,n2) or NULL */, float* rgb /* (n0,n1,n2,3) or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNERF_H */
