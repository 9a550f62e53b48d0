// dpenv_api.hip - host side of libdpenv.so: every entry point of the C ABI (include/dpenv.h) that takes a handle (the others are in
// dpenv_api_free.hip).  Owns the per-env state block in HBM, validates arguments, fills the kernel argument block and launches on the
// caller's stream.  No CPU compute path exists here by design: if HIP or the device is unavailable every entry point fails loudly.
// The handle's struct is defined here and nowhere else: no other unit can look inside a handle.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "dpenv_host.h"

using namespace dpenv;
using namespace dpenv::host;

enum { LOSS_OFF = 0, LOSS_ON = 1, LOSS_UNKNOWN = 2 };
// what allocates the wrench of the baseline's PID in dpenv_controller_rollout: exactly one of these
enum { ALLOC_PINV = 0, ALLOC_QP, ALLOC_QP_TAB, ALLOC_NN };

// A handle owns what it allocates: the destructor releases all of it, so a failed dpenv_create and dpenv_destroy are the same code.
#pragma GCC visibility push(hidden)      // its constructor and destructor are no part of the library's symbol table
struct dpenv_s {
    dpenv_config cfg = {};
    StepArgs args = {};     // persistent part of the kernel argument block
    int mode = 0;
    int n_classes = 1;
    float* blob = nullptr;  // one allocation: S0 | S1 | S2 | RF | episode | vc | beta | class_id | class_tab
    size_t blob_bytes = 0;
    float* cur_vc = nullptr;
    float* cur_beta = nullptr;
    float* cur_vc0 = nullptr;
    float* cur_beta0 = nullptr;
    uint32_t* drift_ctr = nullptr;
    int32_t* class_id = nullptr;
    float4* env_tab = nullptr;   // per-env parameter blocks + thrust-loss rows ET[DRAW_GROUPS][env_stride] (dpenv_dev.h), always allocated
    int env_stride = 0;
    uint32_t* loss_flag = nullptr;   // device word BEHIND the table (ET[DRAW_GROUPS][stride] | flag): the packing kernel reports "some env has a thrust-loss
                            //   coefficient" through it; while the host does not know the answer (LOSS_UNKNOWN) the general per-env kernels run with
                            //   the loss applied: zero coefficients are neutral bit for bit
    int loss_state = LOSS_OFF;   // LOSS_OFF / LOSS_ON / LOSS_UNKNOWN -> StepArgs.loss_on (per-env blocks in force only)
    bool loss_pending = false;   // the flag word is on its way to loss_host behind loss_ev: resolved (without blocking a capture) by the next launch
    hipEvent_t loss_ev = nullptr;
    uint32_t* loss_host = nullptr;   // pinned host word
    bool rand_loss = false; // the randomisation's nominal hull has a thrust-loss coefficient (then every drawn hull has one)
    bool shared_loss = false;   // the SINGLE class of dpenv_create has thrust-loss coefficients: kernels with the shared-loss instantiation take them from
                            //   the arguments (StepArgs.kl, VES_ARGS_LOSS); for the others env_tab holds that hull for every env while no
                            //   per-env table is in force (repacked from raw0_dev when the caller returns to the class)
    float* raw0_dev = nullptr;   // device copy of raw0
    bool cur_rand = false;  // per-episode randomisation of the current (dpenv_set_current_randomisation): needs per-env blocks in force
    float* cur_nom = nullptr;    // device float[2][env_stride]: nominal V_c | beta_c of every env
    float* rand_tab = nullptr;   // device float[RAND_TAB_FLOATS]: nominal | relative half-range of the domain randomisation
    float rand_host[RAND_TAB_FLOATS] = {};   // its host image (the source of the stream-ordered upload must outlive the call)
    float raw0[DPENV_NPARAM] = {};           // public parameter vector of class 0 (the randomisation's default nominal hull)
    bool per_env = false;   // the kernels take every env's vessel from env_tab (dpenv_set_vessel_params / dpenv_set_vessel_randomisation)
    bool randomise = false; // every reset re-draws the env's hull
    bool classes_assigned = false;
    uint32_t* noise_ctr = nullptr;
    PolicyArgs pol = {};    // persistent part (weights, std) of the policy kernel arguments
    void* pol_buf = nullptr;     // fragments | bias tiles | constants, as the kernels stage them: TWO images of pol_buf_bytes / 2 each,
    size_t pol_buf_bytes = 0;    //   written alternately, so that an upload never touches the image the launches before it read
    int pol_slot = 0;       // image the NEXT alternating upload writes (0 / 1)
    int pol_cur = 0;        // image the LAST upload wrote = the one launches read
    hipEvent_t pol_read[2] = {nullptr, nullptr};   // recorded behind the last launch that read image k: the upload that reuses it waits for that
    bool pol_read_valid[2] = {false, false};
    hipStream_t pol_read_stream[2] = {nullptr, nullptr};   // the stream that event was last recorded on (a reader on another stream chains behind it)
    int pol_pinned = -1;    // >= 0: a captured graph reads this image (PolicyArgs.frags is baked into the graph's kernel nodes by value):
                            //   every later upload is written IN PLACE into it, so that a replay sees the latest weights
    PolicyArgs pol_pin_layout = {};   // ... and the kernel node ALSO holds the image's layout and the launch form by value (nent, nblk, ks, n_hidden,
                            //   act, leak, split, critic_f16, ws, ws_groups): what an in-place upload must not change (layout_differs)
    int n_cus = 256;
    float* pol_raw = nullptr;    // device staging of raw fp32 weights for the host-pointer form of set_policy
    size_t pol_raw_bytes = 0;
    int pol_form = DPENV_LAUNCH_AUTO;   // DPENV_LAUNCH_* requested
    bool has_policy = false;
    bool lag_valid = false; // the state block was last written by a closed-loop launch (PolicyArgs.use_lag)
    bool integ_on = false;  // dpenv_set_integral_action: the closed loop runs the *_integ kernels with `integ`
    IntegArgs integ = {};   // its parameters and per-env state (float4 [n]: I | count), allocated by the first dpenv_set_integral_action
    bool reff_on = false;   // dpenv_set_reference_filter: the closed loop runs the *_reff kernels with `reff`
    FilterArgs reff = {};   // its f32 coefficients and per-env state (float4 [3][n]: pos | vel | acc | target), allocated on first use
    bool ctrl_on = false;   // dpenv_set_dp_controller: dpenv_controller_rollout flies the baseline law with `ctrl`
    ControlArgs ctrl = {};  // its numbers and per-env state (float4 [n]: z | pad), allocated by the first dpenv_set_dp_controller
    bool ctrl_tab_on = false;    // dpenv_set_dp_controller_table: env i flies row i of ctrl_tab instead of ctrl's numbers
    float4* ctrl_tab = nullptr;  // the packed per-env controller block (ctrl_tab_float4s(n) float4), allocated by the first dpenv_set_dp_controller_table
    // The allocation stage, ALLOC_*: the pseudo-inverse of `ctrl` (or of ctrl_tab's rows), the QP law with the numbers of `qp`
    // (dpenv_set_qp_allocator) or with row i of qp_tab on env i, qp_tab_iters iterations (dpenv_set_qp_allocator_table), or the network of
    // `nn` (dpenv_set_nn_allocator).  Invariants, kept by the setters (stage_refusal is their one statement) and relied on everywhere else:
    //   ctrl_tab_on => stage == ALLOC_PINV;   stage != ALLOC_PINV => ctrl_on;   qp_scalar => stage is ALLOC_QP or ALLOC_QP_TAB.
    int stage = ALLOC_PINV;
    QpRollout qp = {};      // the QP's numbers and per-env thruster state (float [5][n]), allocated by the first dpenv_set_qp_allocator[_table]
    bool qp_scalar = false; // qp.q holds numbers dpenv_set_qp_allocator set: what dpenv_set_qp_allocator_table(NULL) returns to
    float4* qp_tab = nullptr;    // the packed per-env QP block (qp_tab_float4s(n) float4), allocated by the first dpenv_set_qp_allocator_table
    int32_t qp_tab_iters = 0;
    NnRollout nn = {};      // its constants and the layers' addresses inside nn_img
    float* nn_img = nullptr;     // the zero-padded weight image (NN_IMAGE_FLOATS floats: the largest shape), allocated by the first dpenv_set_nn_allocator
    // dpenv_set_nn_allocator_population: stage == ALLOC_NN with nn_pop.K >= 1 flies network ((env_id_base + i) / envs_per_net) % K of
    // nn_pop_img on env i (K == 0: the one network of `nn`).  Every rule about ALLOC_NN holds for both.
    NnPop nn_pop = {};           // the constants, network 0's layer addresses inside nn_pop_img, K, waves per network and the reduced wave base
    float* nn_pop_img = nullptr; // the zero-padded image of K networks: re-allocated when the shape or K changes
    int32_t nn_pop_shape[4] = {0, 0, 0, 0};   // n_layers, in_dim, H, K of the image in place
    int device = 0;
    std::string err;

    dpenv_s() = default;
    dpenv_s(const dpenv_s&) = delete;                       // (a copy would release the same resources)
    dpenv_s& operator=(const dpenv_s&) = delete;
    ~dpenv_s()              // on the handle's device (dpenv_create has made it current, dpenv_destroy guards it)
    {
        if (blob) (void)hipFree(blob);
        if (pol_buf) (void)hipFree(pol_buf);
        if (pol_raw) (void)hipFree(pol_raw);
        if (integ.state) (void)hipFree(integ.state);
        if (reff.state) (void)hipFree(reff.state);
        if (ctrl.z) (void)hipFree(ctrl.z);
        if (ctrl_tab) (void)hipFree(ctrl_tab);
        if (qp.state) (void)hipFree(qp.state);
        if (qp_tab) (void)hipFree(qp_tab);
        if (nn_img) (void)hipFree(nn_img);
        if (nn_pop_img) (void)hipFree(nn_pop_img);
        for (int k = 0; k < 2; ++k) if (pol_read[k]) (void)hipEventDestroy(pol_read[k]);
        if (loss_ev) (void)hipEventDestroy(loss_ev);
        if (loss_host) (void)hipHostFree(loss_host);
    }
};
#pragma GCC visibility pop

static thread_local std::string g_create_err;

int host::fail(dpenv_handle h, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_err = buf;
    return code;
}

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

extern "C" int dpenv_create(const dpenv_config* cfg, const float* vessel_params, int32_t n_classes, dpenv_handle* out)
{
    if (!cfg || !out) return fail(nullptr, DPENV_EINVAL, "dpenv_create: NULL argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(dpenv_config))
        return fail(nullptr, DPENV_EINVAL, "dpenv_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size,
                    sizeof(dpenv_config));
    if (cfg->n_envs <= 0) return fail(nullptr, DPENV_EINVAL, "n_envs must be positive");
    const int mode = mode_of(cfg);
    if (mode < 0) return fail(nullptr, DPENV_EINVAL, "unknown variant %d", cfg->variant);
    if (cfg->cont_ang && cfg->variant != DPENV_FINAL)
        return fail(nullptr, DPENV_EINVAL, "cont_ang is only defined for the final variant (customEnv.py:228)");
    if (cfg->variant == DPENV_SIMPLE && cfg->extended_state)
        return fail(nullptr, DPENV_EINVAL,
                    "simple + extended_state is not runnable in the reference either (IndexError at customEnv.py:319)");
    if (cfg->n_substeps <= 0 || !(cfg->substep_dt > 0.0f)) return fail(nullptr, DPENV_EINVAL, "bad sub-step settings");
    if (cfg->action_layout < 0 || cfg->action_layout > 1 || cfg->obs_layout < 0 || cfg->obs_layout > 1)
        return fail(nullptr, DPENV_EINVAL, "bad layout");
    if (cfg->obs_dtype != DPENV_F32 && cfg->obs_dtype != DPENV_BF16) return fail(nullptr, DPENV_EINVAL, "bad obs_dtype");
    if (cfg->max_ep_len < 0) return fail(nullptr, DPENV_EINVAL, "max_ep_len < 0");
    if (cfg->current_drift && (!cfg->current_enabled || !(cfg->current_tau > 0.0f) || cfg->current_sigma_v < 0.0f ||
                               cfg->current_sigma_beta < 0.0f))
        return fail(nullptr, DPENV_EINVAL, "current_drift needs current_enabled, tau > 0 and non-negative sigmas");
    if (vessel_params == nullptr) n_classes = 1;
    if (n_classes < 1 || n_classes > MAX_CLASSES)
        return fail(nullptr, DPENV_EINVAL, "n_classes must be in [1, %d]", MAX_CLASSES);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, DPENV_ENODEV, "no HIP device available (%s); libdpenv has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    int dev = cfg->device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return fail(nullptr, DPENV_ENODEV, "hipGetDevice failed");
    } else if (dev >= ndev) {
        return fail(nullptr, DPENV_ENODEV, "device %d out of range (%d devices)", dev, ndev);
    }
    if (hipSetDevice(dev) != hipSuccess) return fail(nullptr, DPENV_ENODEV, "hipSetDevice(%d) failed", dev);

    // every failure from here on is a plain return: the handle releases what it holds by then
    std::unique_ptr<dpenv_s> h(new (std::nothrow) dpenv_s());
    if (!h) return fail(nullptr, DPENV_ENOMEM, "host allocation failed");
    h->cfg = *cfg;
    h->mode = mode;
    h->n_classes = n_classes;
    h->device = dev;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) h->n_cus = prop.multiProcessorCount;
    }

    VesselDev tab[MAX_CLASSES];
    float defp[DPENV_NPARAM];
    dpenv_default_vessel(defp);
    for (int c = 0; c < n_classes; ++c) {
        std::string why;
        const float* p = vessel_params ? vessel_params + (size_t)c * DPENV_NPARAM : defp;
        if (derive_vessel(p, &tab[c], &why, n_classes == 1) != DPENV_OK)
            return fail(nullptr, DPENV_EINVAL, "vessel class %d: %s", c, why.c_str());
        if (c == 0) std::memcpy(h->raw0, p, sizeof h->raw0);
    }

    const size_t n = (size_t)cfg->n_envs;
    const size_t npad = align_up(n, 256);
    size_t off = 0;
    auto carve = [&off](size_t bytes) { const size_t o = off; off += bytes; return o; };     // the blob's layout, in this order
    const size_t o_s0 = carve(npad * 16), o_s1 = carve(npad * 16), o_s2 = carve(npad * 16), o_rf = carve(npad * 16);
    const size_t o_ep = carve(npad * 4), o_vc = carve(npad * 4), o_be = carve(npad * 4), o_v0 = carve(npad * 4), o_b0 = carve(npad * 4);
    const size_t o_dc = carve(npad * 4), o_ci = carve(npad * 4), o_nc = carve(npad * 4);
    const size_t o_s3 = carve(npad * 16);
    const size_t o_ct = carve(align_up(sizeof(VesselDev) * MAX_CLASSES, 256));
    const size_t o_rt = carve(align_up(sizeof(float) * RAND_TAB_FLOATS, 256));
    const size_t o_r0 = carve(256);                                      // raw0_dev
    const size_t o_cn = carve(npad * 4 * 2);                             // cur_nom
    const size_t o_et = carve(npad * 16 * DRAW_GROUPS + 256);            // the per-env table and, behind it, its thrust-loss flag word
    h->blob_bytes = off;
    void* blob = nullptr;
    e = hipMalloc(&blob, off);
    if (e != hipSuccess) return fail(nullptr, DPENV_ENOMEM, "hipMalloc(%zu) failed: %s", off, hipGetErrorString(e));
    h->blob = (float*)blob;
    char* b = (char*)blob;
    e = hipEventCreateWithFlags(&h->loss_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->loss_host, sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) return fail(nullptr, DPENV_EHIP, "event / pinned word of the per-env table's flag: %s", hipGetErrorString(e));
    *h->loss_host = 0u;
    e = hipMemset(blob, 0, off);
    if (e == hipSuccess) e = hipMemcpy(b + o_ct, tab, sizeof(VesselDev) * n_classes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(nullptr, DPENV_EHIP, "state initialisation failed: %s", hipGetErrorString(e));

    StepArgs& a = h->args;
    a.S0 = (float4*)(b + o_s0); a.S1 = (float4*)(b + o_s1); a.S2 = (float4*)(b + o_s2); a.RF = (float4*)(b + o_rf);
    a.episode = (int32_t*)(b + o_ep);
    h->cur_vc = (float*)(b + o_vc); h->cur_beta = (float*)(b + o_be);
    h->cur_vc0 = (float*)(b + o_v0); h->cur_beta0 = (float*)(b + o_b0);
    h->drift_ctr = (uint32_t*)(b + o_dc);
    h->class_id = (int32_t*)(b + o_ci);
    h->noise_ctr = (uint32_t*)(b + o_nc);
    h->env_tab = (float4*)(b + o_et);
    h->env_stride = (int)npad;
    h->rand_tab = (float*)(b + o_rt);
    h->raw0_dev = (float*)(b + o_r0);
    h->cur_nom = (float*)(b + o_cn);
    h->loss_flag = (uint32_t*)(b + o_et + npad * 16 * DRAW_GROUPS);     // = env_tab + DRAW_GROUPS * env_stride: read back by resolve_loss; kernels see StepArgs.loss_on
    a.class_tab = (const float*)(b + o_ct);
    a.n_classes = n_classes;
    a.v0 = tab[0];
    a.n = cfg->n_envs;
    a.n_substeps = cfg->n_substeps;
    a.h = cfg->substep_dt;
    a.inv_dt = 1.0f / (cfg->substep_dt * (float)cfg->n_substeps);
    a.max_ep_len = cfg->max_ep_len;
    a.terminate = cfg->terminate;
    a.auto_reset = cfg->auto_reset;
    a.wrap_mode = cfg->wrap_mode;
    a.action_layout = cfg->action_layout;
    a.obs_layout = cfg->obs_layout;
    a.obs_bf16 = (cfg->obs_dtype == DPENV_BF16);
    a.hold_plant = cfg->hold_plant;
    {
        const float dt = cfg->substep_dt * (float)cfg->n_substeps;
        a.current_drift = cfg->current_drift;
        a.drift_a = cfg->current_drift ? dt / cfg->current_tau : 0.0f;
        a.drift_sv = cfg->current_drift ? cfg->current_sigma_v * sqrtf(2.0f * dt / cfg->current_tau) : 0.0f;
        a.drift_sb = cfg->current_drift ? cfg->current_sigma_beta * sqrtf(2.0f * dt / cfg->current_tau) : 0.0f;
    }
    a.seed_lo = (uint32_t)(cfg->seed & 0xffffffffu);
    a.seed_hi = (uint32_t)(cfg->seed >> 32);
    a.env_id_base = cfg->env_id_base;
    a.reset_fraction = cfg->reset_fraction;
    a.reset_acts = cfg->reset_acts ? 1 : 0;
    a.noise_ctr = h->noise_ctr;
    a.S3 = (float4*)(b + o_s3);
    {
        // a single class WITH thrust-loss coefficients (the thrust-loss preset): the step / fused-rollout kernels and the two-wave closed loop of
        // the shipped configuration have an instantiation that takes hull AND coefficients from the kernel arguments (VES_ARGS_LOSS, round 6);
        // the remaining kernels (one-wave closed loop, other env variants' two-wave forms) carry the loss code in their general per-env form
        // only - for them the table holds this hull for every env
        bool any = false;
        for (int p = 0; p < 3; ++p) {
            a.kl[p] = h->raw0[DPENV_P_KLF_BOW + p]; a.kl[3 + p] = h->raw0[DPENV_P_KLR_BOW + p];
            any = any || a.kl[p] != 0.0f || a.kl[3 + p] != 0.0f;
        }
        e = hipMemcpy(h->raw0_dev, h->raw0, sizeof h->raw0, hipMemcpyHostToDevice);
        if (e == hipSuccess) {       // the table starts as the image of class 0 for every env (what the kernels without a shared form read)
            e = dev::launch_pack_env_vessels(h->raw0_dev, 1, 0, h->env_tab, nullptr, h->env_stride, cfg->n_envs, nullptr);
            if (e == hipSuccess) e = hipDeviceSynchronize();
        }
        if (e != hipSuccess) return fail(nullptr, DPENV_EHIP, "the class hull's device copy / per-env image: %s", hipGetErrorString(e));
        h->shared_loss = any && n_classes == 1;
    }
    *out = h.release();
    return DPENV_OK;
}

extern "C" int dpenv_destroy(dpenv_handle h)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    delete h;
    return DPENV_OK;
}

extern "C" const char* dpenv_last_error(dpenv_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int dpenv_set_reset_fraction(dpenv_handle h, float fraction)
{
    if (!h) return DPENV_EINVAL;
    if (!(fraction >= 0.0f) || !std::isfinite(fraction)) return fail(h, DPENV_EINVAL, "bad reset fraction");
    h->cfg.reset_fraction = fraction;
    h->args.reset_fraction = fraction;
    return DPENV_OK;
}

extern "C" int dpenv_set_vessel_class(dpenv_handle h, const int32_t* class_id, dpenv_stream s)
{
    if (!h || !class_id) return fail(h, DPENV_EINVAL, "dpenv_set_vessel_class: NULL argument");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, hipMemcpyAsync(h->class_id, class_id, sizeof(int32_t) * (size_t)h->cfg.n_envs, hipMemcpyDeviceToDevice,
                              (hipStream_t)s));
    h->classes_assigned = true;
    return DPENV_OK;
}

static int require_current(dpenv_handle h) { return h->cfg.current_enabled ? DPENV_OK : fail(h, DPENV_EINVAL, "config.current_enabled is 0"); }

// The four current accessors are one copy with the pointers permuted: the caller's two arrays against the present values (cur_vc,
// cur_beta), the drift means (cur_vc0, cur_beta0) or, for dpenv_set_current, both in that order.
enum { CUR_SET = 1, CUR_PRESENT = 2, CUR_MEAN = 4 };
static int current_io(dpenv_handle h, const char* who, float* vc, float* beta, int what, dpenv_stream s)
{
    if (!h || !vc || !beta) return fail(h, DPENV_EINVAL, "%s: NULL argument", who);
    DeviceGuard dev_guard(h->device);
    if (int rc = require_current(h)) return rc;
    const size_t bytes = sizeof(float) * (size_t)h->cfg.n_envs;
    float* const theirs[2] = {vc, beta};
    float* const mine[2][2] = {{h->cur_vc, h->cur_beta}, {h->cur_vc0, h->cur_beta0}};
    const bool set = what & CUR_SET;
    for (int k = 0; k < 2; ++k)
        for (int j = 0; j < 2 && (what & (k ? CUR_MEAN : CUR_PRESENT)); ++j)
            HIP_TRY(h, hipMemcpyAsync(set ? mine[k][j] : theirs[j], set ? theirs[j] : mine[k][j], bytes, hipMemcpyDeviceToDevice, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_set_current(dpenv_handle h, const float* vc, const float* beta, dpenv_stream s)
{
    return current_io(h, "dpenv_set_current", (float*)vc, (float*)beta, CUR_SET | CUR_PRESENT | CUR_MEAN, s);
}

extern "C" int dpenv_set_current_present(dpenv_handle h, const float* vc, const float* beta, dpenv_stream s)
{
    return current_io(h, "dpenv_set_current_present", (float*)vc, (float*)beta, CUR_SET | CUR_PRESENT, s);
}

extern "C" int dpenv_get_current(dpenv_handle h, float* vc_out, float* beta_out, dpenv_stream s)
{
    return current_io(h, "dpenv_get_current", vc_out, beta_out, CUR_PRESENT, s);
}

extern "C" int dpenv_get_current_mean(dpenv_handle h, float* vc_out, float* beta_out, dpenv_stream s)
{
    return current_io(h, "dpenv_get_current_mean", vc_out, beta_out, CUR_MEAN, s);
}

extern "C" int dpenv_set_current_randomisation(dpenv_handle h, const float* vc_nominal, const float* beta_nominal, float vc_range,
                                               float beta_range, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (int rc = require_current(h)) return rc;
    if (!(vc_range >= 0.0f) || !(beta_range >= 0.0f) || !std::isfinite(vc_range) || !std::isfinite(beta_range))
        return fail(h, DPENV_EINVAL, "the half-ranges must be finite and >= 0");
    if (vc_range == 0.0f && beta_range == 0.0f) {             // off: every env keeps the current (and the drift mean) it has
        h->cur_rand = false;
        h->args.cur_range_v = h->args.cur_range_b = 0.0f;
        return DPENV_OK;
    }
    if (!h->per_env && h->n_classes > 1)
        return fail(h, DPENV_EINVAL, "the re-draw has no vessel-class form: with vessel classes give every env its block first (dpenv_set_vessel_params)");
    const size_t bytes = sizeof(float) * (size_t)h->cfg.n_envs;
    // NULL: the means in force - unless the randomisation is already on (then the means are drawn values: the nominals stay what they are)
    if (vc_nominal || !h->cur_rand)
        HIP_TRY(h, hipMemcpyAsync(h->cur_nom, vc_nominal ? vc_nominal : h->cur_vc0, bytes, hipMemcpyDeviceToDevice, (hipStream_t)s));
    if (beta_nominal || !h->cur_rand)
        HIP_TRY(h, hipMemcpyAsync(h->cur_nom + h->env_stride, beta_nominal ? beta_nominal : h->cur_beta0, bytes, hipMemcpyDeviceToDevice, (hipStream_t)s));
    h->cur_rand = true;
    h->args.cur_range_v = vc_range;
    h->args.cur_range_b = beta_range;
    return DPENV_OK;
}

// The packing kernel's flag word is on its way to the host (dpenv_set_vessel_params): take it if it has arrived; wait for it unless the launch
// that asks is being RECORDED into a graph - a recorded launch (and every launch after a setter that was itself recorded) runs the general
// per-env kernels with the table's coefficients applied (LOSS_TABLE): where no env has one they are zeros, which leave every row as it is
static bool is_capturing(hipStream_t s)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    return cap != hipStreamCaptureStatusNone;
}

static void resolve_loss(dpenv_handle h, hipStream_t s)
{
    if (!h->loss_pending) return;
    hipError_t q = hipEventQuery(h->loss_ev);
    if (q == hipErrorNotReady) {
        (void)hipGetLastError();                                        // (not an error: the launch below must not report it)
        if (is_capturing(s)) return;
        q = hipEventSynchronize(h->loss_ev);
    }
    if (q != hipSuccess) { (void)hipGetLastError(); return; }            // unknown stays unknown: the loss stays applied
    h->loss_state = *(volatile uint32_t*)h->loss_host != 0u ? LOSS_ON : LOSS_OFF;
    h->loss_pending = false;
}

static void bind_optional(dpenv_handle h, StepArgs& a, hipStream_t s)
{
    // current_enabled without dpenv_set_current = zero current (the block is zero-initialised)
    a.cur_vc = h->cfg.current_enabled ? h->cur_vc : nullptr;
    a.cur_beta = h->cfg.current_enabled ? h->cur_beta : nullptr;
    a.cur_vc0 = h->cur_vc0;
    a.cur_beta0 = h->cur_beta0;
    a.drift_ctr = h->drift_ctr;
    a.class_id = h->class_id;
    resolve_loss(h, s);
    a.env_tab = h->per_env ? h->env_tab : nullptr;
    a.env_stride = h->env_stride;
    // the per-episode current re-draw lives in the general per-env kernels and in the shared training form (one class)
    const bool cr = h->cur_rand && h->cfg.current_enabled && (h->per_env || h->n_classes == 1);
    a.loss_on = h->per_env ? (h->loss_state == LOSS_OFF ? (int)LOSS_NONE : (int)LOSS_TABLE) : ((h->shared_loss || cr) ? (int)LOSS_SHARED : (int)LOSS_NONE);
    a.rand_tab = (h->per_env && h->randomise) ? h->rand_tab : nullptr;
    a.cur_nom = cr ? h->cur_nom : nullptr;
    a.cur_nom_stride = h->env_stride;
}

// a kernel without a shared training form (the one-wave closed loop; the two-wave closed loop of other env variants) on a handle that runs on it:
// the thrust loss through the table image of the class hull (every env the same block) in its general per-env form, or no loss at all; the
// current re-draw is a run-time switch in those kernels whatever the vessel's source
static void bind_shared_loss_as_table(dpenv_handle h, StepArgs& a)
{
    if (a.loss_on != LOSS_SHARED) return;
    if (h->shared_loss) { a.env_tab = h->env_tab; a.loss_on = LOSS_TABLE; }
    else a.loss_on = LOSS_NONE;
}

// where the kernels take a lane's vessel from (dpenv_dev.h VES_*); call after bind_optional (which settles loss_state)
static int vessel_source(dpenv_handle h)
{
    if (h->per_env)
        return (h->randomise || h->loss_state != LOSS_OFF || (h->cur_rand && h->cfg.current_enabled)) ? VES_ENV_RND
               : (h->cfg.per_env_lds ? VES_ENV_LDS : VES_ENV_VGPR);
    if (h->n_classes > 1) return VES_CLASS_LDS;
    return (h->shared_loss || (h->cur_rand && h->cfg.current_enabled)) ? VES_ARGS_LOSS : VES_ARGS;
}

// a device block of a feature (integral action, reference filter, DP controller and its table, QP allocator and its table, NN image):
// allocated by the first call that turns the feature on, kept while it is off, released with the handle
template <class T>
static int ensure_block(dpenv_handle h, T** block, size_t bytes, const char* msg)
{
    if (*block) return DPENV_OK;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return fail(h, DPENV_ENOMEM, "%s", msg);
    *block = (T*)p;
    return DPENV_OK;
}
static size_t env_bytes(dpenv_handle h, size_t per_env) { return per_env * (size_t)h->cfg.n_envs; }

static bool qp_flies(dpenv_handle h) { return h->stage == ALLOC_QP || h->stage == ALLOC_QP_TAB; }

static int require_classes(dpenv_handle h)
{
    if (!h->per_env && h->n_classes > 1 && !h->classes_assigned)
        return fail(h, DPENV_EINVAL, "n_classes > 1 but dpenv_set_vessel_class was never called");
    return DPENV_OK;
}

// the setpoint schedule of a T-step launch: dpenv_rollout_io, dpenv_policy_rollout_io and dpenv_controller_rollout_io carry the same fields
template <class IO>
static int check_schedule(dpenv_handle h, const IO* io)
{
    if (io->n_switch < 0 || io->n_switch > DPENV_MAX_SWITCH || (io->n_switch > 0 && !io->refs))
        return fail(h, DPENV_EINVAL, "bad setpoint schedule");
    for (int k = 0; k < io->n_switch; ++k)
        if (io->switch_step[k] < 0 || io->switch_step[k] >= io->T || (k > 0 && io->switch_step[k] <= io->switch_step[k - 1]))
            return fail(h, DPENV_EINVAL, "switch_step must be strictly increasing within [0, T)");
    return DPENV_OK;
}

// ... into the launch's argument block (RolloutArgs, PolicyArgs, ControlArgs)
template <class IO, class Args>
static void copy_schedule(const IO* io, Args& a)
{
    a.n_switch = io->n_switch;
    a.refs = io->refs;
    for (int k = 0; k < io->n_switch; ++k) a.switch_step[k] = io->switch_step[k];
}

// ---- per-env parameter blocks ------------------------------------------------------------------------------------------------
extern "C" int dpenv_set_vessel_params_ex(dpenv_handle h, const float* params, uint32_t flags, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    // everything that can refuse the call comes first; the handle's switches (per_env, randomise, loss_state) change only after the last
    // call that can fail (ADVICE / VERDICT r05: a refused call used to leave the thrust loss and the re-draws silently off)
    if (flags & ~(uint32_t)DPENV_VESSEL_KEEP_RANDOMISATION) return fail(h, DPENV_EINVAL, "dpenv_set_vessel_params_ex: unknown flag bits 0x%x", flags);
    const bool keep = (flags & DPENV_VESSEL_KEEP_RANDOMISATION) != 0;
    if (keep && (!params || !h->randomise))
        return fail(h, DPENV_EINVAL, "DPENV_VESSEL_KEEP_RANDOMISATION needs a table and the randomisation in force (dpenv_set_vessel_randomisation first)");
    if (!params) {
        if (h->cur_rand && h->n_classes > 1)
            return fail(h, DPENV_EINVAL, "the per-episode current randomisation has no vessel-class form: switch it off first "
                                         "(dpenv_set_current_randomisation with both ranges 0)");
        // back to the classes / the single class; a single class WITH thrust-loss coefficients keeps them (kernel arguments), and the table
        // becomes the image of that hull again for the kernels that read it there
        if (h->per_env)
            HIP_TRY(h, dev::launch_pack_env_vessels(h->raw0_dev, 1, 0, h->env_tab, nullptr, h->env_stride, h->cfg.n_envs, (hipStream_t)s));
        h->per_env = false;
        h->randomise = false;
        h->loss_pending = false;
        h->loss_state = LOSS_OFF;
        return DPENV_OK;
    }
    const bool capturing = is_capturing((hipStream_t)s);
    // stream-ordered, no read-back: the packing kernel leaves "some env has a thrust-loss coefficient" in the word behind the table
    HIP_TRY(h, hipMemsetAsync(h->loss_flag, 0, sizeof(uint32_t), (hipStream_t)s));
    HIP_TRY(h, dev::launch_pack_env_vessels(params, (int64_t)h->cfg.n_envs, 1, h->env_tab, h->loss_flag, h->env_stride, h->cfg.n_envs, (hipStream_t)s));
    // which kernels run from here on depends on that word (the general per-env form applies the loss, the plain one does not carry the code).
    // Outside a capture it also travels to a pinned host word behind an event: the next launch takes the answer from there (resolve_loss);
    // recorded into a graph the setter leaves the answer unknown: the general kernels then apply the table's coefficients whatever they are.
    bool pending = false;
    if (!capturing) {
        HIP_TRY(h, hipMemcpyAsync(h->loss_host, h->loss_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)s));
        HIP_TRY(h, hipEventRecord(h->loss_ev, (hipStream_t)s));
        pending = true;
    }
    h->per_env = true;
    if (!keep) h->randomise = false;
    if (h->randomise && h->rand_loss) { h->loss_state = LOSS_ON; h->loss_pending = false; }     // every drawn hull has a coefficient: nothing to ask
    else { h->loss_state = LOSS_UNKNOWN; h->loss_pending = pending; }
    return DPENV_OK;
}

extern "C" int dpenv_set_vessel_params(dpenv_handle h, const float* params, dpenv_stream s)
{
    return dpenv_set_vessel_params_ex(h, params, 0u, s);
}

extern "C" int dpenv_get_vessel_params(dpenv_handle h, float* params_out, dpenv_stream s)
{
    if (!h || !params_out) return fail(h, DPENV_EINVAL, "dpenv_get_vessel_params: NULL argument");
    if (!h->per_env && h->n_classes > 1)
        return fail(h, DPENV_EINVAL, "no per-env parameter blocks in force (dpenv_set_vessel_params / dpenv_set_vessel_randomisation)");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_unpack_env_vessels(h->env_tab, h->env_stride, params_out, h->cfg.n_envs, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_set_vessel_randomisation(dpenv_handle h, const float* nominal, const float* rel_range, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (!rel_range) { h->randomise = false; return DPENV_OK; }         // hulls stay as they are, no more re-draws
    const float* nom = nominal ? nominal : h->raw0;
    for (int p = 0; p < DPENV_NPARAM; ++p) {
        const float r = p < RAND_NPARAM ? rel_range[p] : 0.0f;
        if (!std::isfinite(nom[p]) || !(r >= 0.0f && r < 1.0f) || (p >= DPENV_P_KLF_BOW && nom[p] < 0.0f))
            return fail(h, DPENV_EINVAL, "parameter %d: nominal must be finite (thrust-loss coefficients >= 0) and the relative half-range in [0, 1)", p);
        h->rand_host[p] = nom[p];
        h->rand_host[32 + p] = r;
    }
    {
        // every hull the draw can produce must be a vessel: the corner of the range with the lightest diagonal and the largest coupling
        const double m11 = (double)nom[DPENV_P_M11] * (1.0 - rel_range[DPENV_P_M11]);
        const double m22 = (double)nom[DPENV_P_M22] * (1.0 - rel_range[DPENV_P_M22]);
        const double m33 = (double)nom[DPENV_P_M33] * (1.0 - rel_range[DPENV_P_M33]);
        const double m23 = std::fabs((double)nom[DPENV_P_M23]) * (1.0 + rel_range[DPENV_P_M23]);
        if (!(m11 > 0.0) || !(m22 > 0.0) || !(m22 * m33 - m23 * m23 > 0.0))
            return fail(h, DPENV_EINVAL, "the range admits a mass matrix that is not positive definite");
    }
    HIP_TRY(h, hipMemcpyAsync(h->rand_tab, h->rand_host, sizeof h->rand_host, hipMemcpyHostToDevice, (hipStream_t)s));
    // until its first reset every env runs on the nominal hull
    HIP_TRY(h, dev::launch_pack_env_vessels(h->rand_tab, 1, 0, h->env_tab, nullptr, h->env_stride, h->cfg.n_envs, (hipStream_t)s));
    h->per_env = true;
    h->randomise = true;
    h->rand_loss = false;                               // a draw scales the nominal value: no coefficient there, none in any hull
    for (int p = DPENV_P_KLF_BOW; p <= DPENV_P_KLR_STAR; ++p) h->rand_loss = h->rand_loss || nom[p] != 0.0f;
    h->loss_state = h->rand_loss ? LOSS_ON : LOSS_OFF;
    h->loss_pending = false;
    return DPENV_OK;
}

extern "C" int dpenv_reset(dpenv_handle h, const uint8_t* mask, const float* init, const float* ref, void* obs_out,
                           dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    StepArgs a = h->args;
    bind_optional(h, a, (hipStream_t)s);
    a.obs = obs_out;
    HIP_TRY(h, dev::launch_reset(&a, h->mode, h->cfg.extended_state, mask, init, ref, (hipStream_t)s));
    if (h->integ_on) HIP_TRY(h, dev::launch_integ_clear(h->integ.state, mask, h->cfg.n_envs, (hipStream_t)s));   // new episodes start with I = 0
    if (h->reff_on) HIP_TRY(h, dev::launch_reff_rest(a.RF, h->reff.state, mask, h->cfg.n_envs, (hipStream_t)s));   // ... the filter at rest
    if (h->ctrl_on) HIP_TRY(h, dev::launch_control_state(h->ctrl.z, nullptr, mask, h->cfg.n_envs, 2, (hipStream_t)s));   // ... the baseline's z = 0
    if (qp_flies(h)) HIP_TRY(h, dev::launch_qp_state_clear(h->qp.state, mask, h->cfg.n_envs, (hipStream_t)s));               // ... and its QP allocator's thrusters at rest
    // the reset kernel writes the lagged thrust columns (S3) of the envs it re-draws: a full reset makes them valid everywhere, a
    // masked one leaves the validity of the other envs' columns as it was (it used to drop the lag of every env)
    if (!mask) h->lag_valid = true;
    return DPENV_OK;
}

#define INTEG_OPEN_LOOP_MSG                                                                                                         \
    "%s: the integral action is on (dpenv_set_integral_action) and this launch's observations would lack I: run the closed loop "    \
    "(dpenv_policy_rollout), compose the step with the law on the host, or turn the action off"
#define REFF_OPEN_LOOP_MSG                                                                                                          \
    "%s: the reference filter is on (dpenv_set_reference_filter) and would not see this launch: run the closed loop "               \
    "(dpenv_policy_rollout), compose the step with the filter on the host (its position as new_ref), or turn the filter off"

extern "C" int dpenv_step_ex(dpenv_handle h, const dpenv_step_io* io, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (!io || io->struct_size != sizeof(dpenv_step_io)) return fail(h, DPENV_EINVAL, "dpenv_step_io ABI mismatch");
    if (h->integ_on) return fail(h, DPENV_EINVAL, INTEG_OPEN_LOOP_MSG, "dpenv_step");
    if (h->reff_on) return fail(h, DPENV_EINVAL, REFF_OPEN_LOOP_MSG, "dpenv_step");
    if (!io->action || !io->obs || !io->reward || !io->done)
        return fail(h, DPENV_EINVAL, "action, obs, reward and done buffers are required");
    if (int rc = require_classes(h)) return rc;
    StepArgs a = h->args;
    bind_optional(h, a, (hipStream_t)s);
    a.action = io->action;
    a.new_ref = io->new_ref;
    a.obs = io->obs;
    a.rew = io->reward;
    a.done = io->done;
    a.parts = io->reward_parts;
    a.final_obs = io->final_obs;
    // the lagged thrust columns (S3) are kept by every kernel that changes the state; the one-launch-per-step kernel writes them only
    // while a policy is in force (16 B per env-step more) - without one the columns are marked stale and a later closed-loop launch
    // rebuilds its first observation from the state block
    if (!h->has_policy) a.S3 = nullptr;
    // the reset wave pays while the batch leaves it a SIMD slot beside its env wave (<= one env wave per SIMD = 256 envs per CU: 65 536 on
    // MI355X); beyond that the extra waves queue behind env waves and the one-wave kernel is faster (98 304 envs: 6.92 vs 7.19 us, 1 M:
    // 34.7 vs 39.2; profiles/r04_reset_wave.txt)
    const int reset_wave = (!h->cfg.step_one_wave && (int64_t)h->cfg.n_envs <= (int64_t)256 * h->n_cus) ? 1 : 0;
    HIP_TRY(h, dev::launch_step(&a, h->mode, h->cfg.extended_state, vessel_source(h), reset_wave, (hipStream_t)s));
    h->lag_valid = h->has_policy;
    return DPENV_OK;
}

extern "C" int dpenv_step(dpenv_handle h, const float* action, const float* new_ref, void* obs_out, float* rew_out,
                          uint8_t* done_out, dpenv_stream s)
{
    dpenv_step_io io = {};
    io.struct_size = (uint32_t)sizeof io;
    io.action = action; io.new_ref = new_ref; io.obs = obs_out; io.reward = rew_out; io.done = done_out;
    return dpenv_step_ex(h, &io, s);
}

extern "C" int dpenv_rollout(dpenv_handle h, const dpenv_rollout_io* io, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (!io || io->struct_size != sizeof(dpenv_rollout_io)) return fail(h, DPENV_EINVAL, "dpenv_rollout_io ABI mismatch");
    if (h->integ_on) return fail(h, DPENV_EINVAL, INTEG_OPEN_LOOP_MSG, "dpenv_rollout");
    if (h->reff_on) return fail(h, DPENV_EINVAL, REFF_OPEN_LOOP_MSG, "dpenv_rollout");
    if (io->T <= 0 || !io->actions || !io->obs || !io->reward || !io->done)
        return fail(h, DPENV_EINVAL, "T > 0 and action, obs, reward, done blocks are required");
    if (int rc = check_schedule(h, io)) return rc;
    if (int rc = require_classes(h)) return rc;
    StepArgs a = h->args;
    bind_optional(h, a, (hipStream_t)s);
    RolloutArgs ra = {};
    ra.T = io->T; ra.actions = io->actions; ra.obs = io->obs; ra.rew = io->reward; ra.done = io->done;
    copy_schedule(io, ra);
    // env wave + row wave while the chip has issue slots to spare (measured: 16 384 ... 98 304 envs 5-20 % faster, 131 072 equal, 262 144 and
    // above 10-15 % slower than one wave per 64 envs: profiles/r04_fused_two_wave.txt, r04_batch_sweep.txt)
    // (the randomisation's instantiation needs 201 VGPRs: two waves per SIMD, i.e. up to 256 envs per CU)
    const int two_wave = (!h->cfg.step_one_wave && (int64_t)h->cfg.n_envs <= (int64_t)(vessel_source(h) == VES_ENV_RND ? 256 : 384) * h->n_cus) ? 1 : 0;
    HIP_TRY(h, dev::launch_rollout(&a, &ra, h->mode, h->cfg.extended_state, vessel_source(h), two_wave, (hipStream_t)s));
    // the rollout kernels leave the thrust columns of their last observation in S3 - with the extended state (without it no observation has
    // thrust columns and S3 is never written: the flag keeps what it was)
    if (h->cfg.extended_state) h->lag_valid = true;
    return DPENV_OK;
}

// ---- actor-critic ------------------------------------------------------------------------------------------
static int check_net(const dpenv_mlp* m, int in_dim, int out_dim, std::string* why)
{
    const int nl = m->n_layers;
    if (nl < 2 || nl > 5) { *why = "n_layers must be in [2, 5]"; return DPENV_EINVAL; }
    const int H = m->sizes[1];
    if (m->sizes[0] != in_dim || m->sizes[nl] != out_dim) { *why = "network input/output width does not match the env"; return DPENV_EINVAL; }
    if (in_dim > 15 || out_dim > 8 || H < 1 || H > 96) { *why = "limits: obs_dim <= 15, out <= 8, hidden width <= 96"; return DPENV_EINVAL; }
    for (int l = 1; l < nl; ++l) if (m->sizes[l] != H) { *why = "hidden widths must be equal"; return DPENV_EINVAL; }
    for (int l = 0; l < nl; ++l) if (!m->W[l] || !m->b[l]) { *why = "NULL weight pointer"; return DPENV_EINVAL; }
    return DPENV_OK;
}

// What an upload's shape, arithmetic, activation and launch form come to: the part of PolicyArgs a kernel node holds by value (the image's
// layout - FragAddr, dpenv_policy_dev.h - and the launch form AUTO resolves to; the other fields zero) and the LDS footprint in either form
struct PolicyLayout {
    PolicyArgs pa;          // nent, nblk, ks, n_hidden, act, leak, split, critic_f16, ws, ws_groups
    size_t bytes_frags, bytes_bias, lds_image, lds_two;
    bool form_two, fits_one, fits_two;
};

static PolicyLayout policy_layout(const dpenv_policy_desc* d, int n_envs, int n_cus)
{
    PolicyLayout L = {};
    PolicyArgs& p = L.pa;
    const int H = d->pi->sizes[1];
    p.n_hidden = d->pi->n_layers - 1;
    p.ks = H <= 80 ? 5 : 6;
    p.nent = (128 + (p.ks == 5 ? 32 : 64)) + (p.n_hidden - 1) * p.ks * (128 + (p.ks == 5 ? 32 : 64)) + p.ks * 16;
    p.nblk = 3 * (p.n_hidden - 1) + 1;
    p.act = d->activation;
    p.leak = d->leak;
    p.split = d->precision != DPENV_POLICY_F16;
    p.critic_f16 = d->precision == DPENV_POLICY_F32_ACTOR;
    L.bytes_frags = (size_t)2 * p.nent * 16 * (1 + p.split);
    L.bytes_bias = (size_t)2 * p.nblk * 32 * sizeof(float);
    // the launch form decides the LDS footprint.  The two-wave form stages the images its network wave reads (f16: actor + critic;
    // F32_ACTOR: + the actor's low image; F32: all four) and a mailbox group per 64 envs; it exists for leaky-relu / relu in every
    // arithmetic and for tanh in f16.
    const size_t per_image = (size_t)p.nent * 16, lds_max = 160 * 1024;
    const int n_img_two = !p.split ? 2 : (p.critic_f16 ? 3 : 4);
    L.lds_image = L.bytes_frags + L.bytes_bias;
    L.lds_two = n_img_two * per_image + L.bytes_bias + (p.split ? POLICY_WS_MAILBOX_X_BYTES : POLICY_WS_MAILBOX_BYTES);
    L.form_two = !p.split || d->activation == DPENV_ACT_LEAKY_RELU;
    L.fits_two = L.form_two && L.lds_two <= lds_max;
    L.fits_one = L.lds_image + (p.split ? 0 : POLICY_STAGING_BYTES) <= lds_max;
    // AUTO: the two-wave form where it exists and fits (the faster one), else one wave per 64 envs
    p.ws = d->launch_form == DPENV_LAUNCH_TWO_WAVE ? 1 : (d->launch_form == DPENV_LAUNCH_ONE_WAVE ? 0 : (L.fits_two ? 1 : 0));
    // two-wave geometry: 128-env workgroups (a SIMD per wave) while one round of them fits the chip, else 256-env workgroups;
    // tanh has the 256-env form only
    p.ws_groups = (d->activation == DPENV_ACT_LEAKY_RELU && (n_envs + 127) / 128 <= n_cus) ? 2 : 4;
    return L;
}

// a captured kernel node holds these BY VALUE next to the image's address (dpenv_s::pol_pin_layout): an in-place upload that changed one
// of them would be read with the old layout - wrong weights and no error
static bool layout_differs(const PolicyArgs& q, const PolicyArgs& p)
{
    return q.nent != p.nent || q.nblk != p.nblk || q.ks != p.ks || q.n_hidden != p.n_hidden || q.act != p.act || q.leak != p.leak ||
           q.split != p.split || q.critic_f16 != p.critic_f16 || q.ws != p.ws || q.ws_groups != p.ws_groups;
}

// host weights: staged raw in device memory by stream-ordered copies (pn and *ls_dev point into the staging), then packed on the device
// like the other form
static int stage_host_weights(dpenv_handle h, const dpenv_policy_desc* d, int ad, PackNet pn[2], const float** ls_dev, hipStream_t s)
{
    const int nl = d->pi->n_layers;
    size_t raw = 8;
    for (int k = 0; k < 2; ++k) {
        const dpenv_mlp* m = k ? d->v : d->pi;
        for (int l = 0; l < nl; ++l) raw += (size_t)m->sizes[l] * m->sizes[l + 1] + m->sizes[l + 1];
    }
    // the staging area is reused by every host-pointer upload: the previous one's packing kernel must be done with it (this
    // form is synchronous anyway, see the end of dpenv_set_policy_desc)
    if (h->pol_raw && h->pol_raw_bytes < raw * sizeof(float)) { HIP_TRY(h, hipDeviceSynchronize()); (void)hipFree(h->pol_raw); h->pol_raw = nullptr; }
    if (!h->pol_raw) {
        void* p = nullptr;
        if (hipMalloc(&p, raw * sizeof(float)) != hipSuccess) return fail(h, DPENV_ENOMEM, "hipMalloc of the weight staging failed");
        h->pol_raw = (float*)p; h->pol_raw_bytes = raw * sizeof(float);
    }
    float* cursor = h->pol_raw;
    HIP_TRY(h, hipMemcpyAsync(cursor, d->log_std, sizeof(float) * ad, hipMemcpyHostToDevice, s));
    *ls_dev = cursor; cursor += 8;
    for (int k = 0; k < 2; ++k) {
        const dpenv_mlp* m = k ? d->v : d->pi;
        for (int l = 0; l < nl; ++l) {
            const size_t nw = (size_t)m->sizes[l] * m->sizes[l + 1], nb = m->sizes[l + 1];
            HIP_TRY(h, hipMemcpyAsync(cursor, m->W[l], nw * sizeof(float), hipMemcpyHostToDevice, s));
            pn[k].W[l] = cursor; cursor += nw;
            HIP_TRY(h, hipMemcpyAsync(cursor, m->b[l], nb * sizeof(float), hipMemcpyHostToDevice, s));
            pn[k].b[l] = cursor; cursor += nb;
        }
    }
    return DPENV_OK;
}

extern "C" int dpenv_set_policy_desc(dpenv_handle h, const dpenv_policy_desc* d, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!d || d->struct_size != sizeof(dpenv_policy_desc)) return fail(h, DPENV_EINVAL, "dpenv_policy_desc ABI mismatch");
    if (d->activation != DPENV_ACT_LEAKY_RELU && d->activation != DPENV_ACT_TANH)
        return fail(h, DPENV_EINVAL, "activation must be DPENV_ACT_LEAKY_RELU or DPENV_ACT_TANH");
    if (d->precision != DPENV_POLICY_F16 && d->precision != DPENV_POLICY_F32 && d->precision != DPENV_POLICY_F32_ACTOR)
        return fail(h, DPENV_EINVAL, "bad precision");
    if (d->launch_form < DPENV_LAUNCH_AUTO || d->launch_form > DPENV_LAUNCH_TWO_WAVE) return fail(h, DPENV_EINVAL, "bad launch_form");
    if (d->activation == DPENV_ACT_LEAKY_RELU && !(d->leak >= 0.0f && d->leak <= 1.0f))
        return fail(h, DPENV_EINVAL, "leaky-relu slope must be in [0, 1] (evaluated as max(x, leak x))");
    DeviceGuard dev_guard(h->device);
    const dpenv_mlp* pi = d->pi;
    const dpenv_mlp* v = d->v;
    if (!pi || !v || !d->log_std) return fail(h, DPENV_EINVAL, "dpenv_set_policy: NULL argument");
    if (pi->n_layers != v->n_layers || pi->sizes[1] != v->sizes[1])
        return fail(h, DPENV_EINVAL, "actor and critic must have the same hidden shape");
    const int od = dpenv_obs_dim(&h->cfg), ad = dpenv_act_dim(&h->cfg);
    std::string why;
    if (check_net(pi, od, ad, &why) != DPENV_OK) return fail(h, DPENV_EINVAL, "actor: %s", why.c_str());
    if (check_net(v, od, 1, &why) != DPENV_OK) return fail(h, DPENV_EINVAL, "critic: %s", why.c_str());
    const int nl = pi->n_layers, H = pi->sizes[1];
    // refuse here what the rollout could not launch
    const PolicyLayout L = policy_layout(d, h->cfg.n_envs, h->n_cus);
    if (!L.fits_one) return fail(h, DPENV_EINVAL, "networks do not fit the 160 KiB LDS (%zu bytes of fragments and biases)", L.lds_image);
    if (d->launch_form == DPENV_LAUNCH_TWO_WAVE && !L.fits_two)
        return fail(h, DPENV_EINVAL, L.form_two ? "networks + the two-wave form's mailboxes exceed the 160 KiB LDS (%zu bytes): use DPENV_LAUNCH_ONE_WAVE"
                                                : "the split arithmetics have a two-wave form for leaky-relu / relu only (%zu)", L.lds_two);
    // two images, written alternately: launches issued before this call keep reading the one they were given (the header's
    // promise), whatever stream they run on; the image written now was last read by launches issued before the PREVIOUS upload,
    // and this stream waits for the last of them (an event recorded behind every launch that reads an image).
    const size_t need = (L.bytes_frags + L.bytes_bias + 24 * sizeof(float) + 255) / 256 * 256;
    if (h->pol_buf && h->pol_buf_bytes < 2 * need) {
        // growing the images: a launch that still reads the old ones may be in flight
        HIP_TRY(h, hipDeviceSynchronize());
        (void)hipFree(h->pol_buf); h->pol_buf = nullptr; h->pol_buf_bytes = 0;
        h->has_policy = false;
        h->pol = {};
        h->pol_read_valid[0] = h->pol_read_valid[1] = false;
        h->pol_pinned = -1;                                   // graphs captured on the old images are void (dpenv.h)
    }
    if (!h->pol_buf) {
        if (hipMalloc(&h->pol_buf, 2 * need) != hipSuccess) {
            h->pol_buf = nullptr;                             // (a handle without images has no policy: see above, or it never had one)
            return fail(h, DPENV_ENOMEM, "hipMalloc of the policy images failed");
        }
        h->pol_buf_bytes = 2 * need;
        h->pol_slot = 0;
    }
    const bool capturing = is_capturing((hipStream_t)s);            // inside a captured graph the graph's own edges order everything
    // Which image this upload writes.  Eager launches read the image the last upload wrote (h->pol), so uploads alternate and a launch
    // in flight keeps its weights.  A launch RECORDED INTO A GRAPH has the image's address baked into its kernel node: once that has
    // happened (pol_pinned) an alternating upload would leave every second set of weights invisible to the replays - so from then on
    // every eager upload goes in place into the pinned image, ordered behind the eager readers by their event and behind graph
    // replays by stream order (the caller replays and uploads on one stream, or orders them itself: dpenv.h).
    //  An upload recorded INTO a graph after an image has been pinned goes into the pinned image as well: alternating there would
    // pin the other image at the next captured launch, and the graphs captured first would stop seeing uploads.
    const int slot = (h->pol_pinned >= 0) ? h->pol_pinned : h->pol_slot;
    // Refused while pinned; dpenv_release_policy_graphs() ends the pin once the graphs are gone.
    if (h->pol_pinned >= 0 && layout_differs(h->pol_pin_layout, L.pa))
        return fail(h, DPENV_EINVAL, "a captured graph reads the policy image with another layout (hidden shape, precision, activation, leak or launch "
                                     "form differ): destroy the graphs and call dpenv_release_policy_graphs() before uploading this policy");
    if (!capturing && h->pol_read_valid[slot]) HIP_TRY(h, hipStreamWaitEvent((hipStream_t)s, h->pol_read[slot], 0));
    PackNet pn[2];
    const float* ls_dev = d->log_std;
    if (!d->device_pointers) {
        if (int rc = stage_host_weights(h, d, ad, pn, &ls_dev, (hipStream_t)s)) return rc;
    } else {
        for (int k = 0; k < 2; ++k) {
            const dpenv_mlp* m = k ? v : pi;
            for (int l = 0; l < nl; ++l) { pn[k].W[l] = m->W[l]; pn[k].b[l] = m->b[l]; }
        }
    }
    for (int k = 0; k < 2; ++k) {
        pn[k].n_layers = nl; pn[k].in_dim = od; pn[k].H = H; pn[k].out_dim = k ? 1 : ad;
        for (int l = nl; l < 5; ++l) { pn[k].W[l] = nullptr; pn[k].b[l] = nullptr; }
    }
    char* base = (char*)h->pol_buf + (size_t)slot * (h->pol_buf_bytes / 2);
    float* bias = (float*)(base + L.bytes_frags);
    float* consts = (float*)(base + L.bytes_frags + L.bytes_bias);
    HIP_TRY(h, dev::launch_pack_policy(&pn[0], &pn[1], ls_dev, ad, L.pa.ks, L.pa.nent, L.pa.nblk, L.pa.split, base, bias, consts, (hipStream_t)s));
    h->pol = L.pa;
    h->pol.frags = (const uint4*)base;
    h->pol.bias = bias;
    h->pol.consts = consts;
    h->pol_form = d->launch_form;
    h->has_policy = true;
    h->pol_cur = slot;                                       // "current" = the image just written (pinned or not)
    h->pol_slot = slot ^ 1;
    // host pointers: the caller's arrays (and the shared staging area) must be done with before this returns
    if (!d->device_pointers && !capturing) HIP_TRY(h, hipStreamSynchronize((hipStream_t)s));
    return DPENV_OK;
}

// behind every launch that reads the current image: the event an upload into that image waits for
static int mark_policy_read(dpenv_handle h, dpenv_stream s)
{
    const int cur = h->pol_cur;                             // the image the last upload wrote
    if (is_capturing((hipStream_t)s)) {
        h->pol_pinned = cur;                                // a graph now holds this image's address: uploads go in place from here on
        h->pol_pin_layout = h->pol;                         // ... and its layout / launch form, by value
        return DPENV_OK;
    }
    if (!h->pol_read[cur] && hipEventCreateWithFlags(&h->pol_read[cur], hipEventDisableTiming) != hipSuccess) {
        h->pol_read[cur] = nullptr;
        return fail(h, DPENV_EHIP, "hipEventCreate failed");
    }
    // one event per image: a reader on ANOTHER stream than the last one first waits (on its stream) for the event as it stands, so
    // that the re-recorded event completes only when both readers are done - the chain covers every reader on any stream
    if (h->pol_read_valid[cur] && h->pol_read_stream[cur] != (hipStream_t)s)
        HIP_TRY(h, hipStreamWaitEvent((hipStream_t)s, h->pol_read[cur], 0));
    HIP_TRY(h, hipEventRecord(h->pol_read[cur], (hipStream_t)s));
    h->pol_read_valid[cur] = true;
    h->pol_read_stream[cur] = (hipStream_t)s;
    return DPENV_OK;
}

extern "C" int dpenv_set_policy_ex(dpenv_handle h, const dpenv_mlp* pi, const dpenv_mlp* v, const float* log_std, int32_t activation,
                                   float leak)
{
    dpenv_policy_desc d = {};
    d.struct_size = (uint32_t)sizeof d;
    d.pi = pi; d.v = v; d.log_std = log_std; d.activation = activation; d.leak = leak;
    d.precision = DPENV_POLICY_F16; d.launch_form = DPENV_LAUNCH_AUTO; d.device_pointers = 0;
    const int rc = dpenv_set_policy_desc(h, &d, nullptr);     // host pointers: synchronises the null stream before it returns
    if (rc != DPENV_OK) return rc;
    // the convenience forms keep the contract they always had: when they return the new weights are in force for launches on
    // ANY stream (non-blocking streams do not order themselves behind the null stream)
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, hipDeviceSynchronize());
    return DPENV_OK;
}

extern "C" int dpenv_set_policy(dpenv_handle h, const dpenv_mlp* pi, const dpenv_mlp* v, const float* log_std, float leak)
{
    return dpenv_set_policy_ex(h, pi, v, log_std, DPENV_ACT_LEAKY_RELU, leak);
}

extern "C" int dpenv_get_policy_launch(dpenv_handle h, int32_t* two_wave_out, int32_t* envs_per_workgroup_out)
{
    if (!h) return DPENV_EINVAL;
    if (!h->has_policy) return fail(h, DPENV_EINVAL, "dpenv_set_policy has not been called");
    if (two_wave_out) *two_wave_out = h->pol.ws ? 1 : 0;
    if (envs_per_workgroup_out) *envs_per_workgroup_out = h->pol.ws ? 64 * h->pol.ws_groups : 256;
    return DPENV_OK;
}

static int policy_prec(const PolicyArgs& pa) { return !pa.split ? PREC_F16 : (pa.critic_f16 ? PREC_F32_ACTOR : PREC_F32); }

extern "C" int dpenv_get_policy_launch_ex(dpenv_handle h, int32_t out[4])
{
    if (!h || !out) return fail(h, DPENV_EINVAL, "dpenv_get_policy_launch_ex: NULL argument");
    if (!h->has_policy) return fail(h, DPENV_EINVAL, "dpenv_set_policy has not been called");
    const PolicyArgs& pa = h->pol;
    const int prec = policy_prec(pa);
    out[0] = pa.ws ? 1 : 0;
    out[1] = pa.ws ? 64 * pa.ws_groups : 256;
    out[2] = pa.ws ? ws_roles(prec, pa.ws_groups) : 1;      // waves per 64 envs
    out[3] = prec;
    return DPENV_OK;
}

extern "C" int dpenv_release_policy_graphs(dpenv_handle h)
{
    if (!h) return DPENV_EINVAL;
    h->pol_pinned = -1;                                      // uploads alternate between the two images again
    return DPENV_OK;
}

extern "C" int dpenv_policy_forward(dpenv_handle h, const float* obs, float* mu_out, float* v_out, int32_t n, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (!h->has_policy) return fail(h, DPENV_EINVAL, "dpenv_set_policy has not been called");
    if (!obs || !mu_out || !v_out || n <= 0) return fail(h, DPENV_EINVAL, "dpenv_policy_forward: bad argument");
    const auto forward = h->pol.split ? dev::launch_policy_forward_x : dev::launch_policy_forward;
    HIP_TRY(h, forward(&h->pol, dpenv_obs_dim(&h->cfg), dpenv_act_dim(&h->cfg), obs, mu_out, v_out, n, (hipStream_t)s));
    return mark_policy_read(h, s);
}

// Which closed-loop kernel runs: the one place that decides.  The two-wave form runs where its launcher has the instantiation (the ws_*
// predicates of dpenv_dev.h, the same ones it instantiates by); everything else runs the one-wave kernels - the same rows bit for bit, the
// hull / current re-draw and the table's thrust loss a run-time switch there, which know the thrust loss through the table alone.
#define ONE_WAVE_SET_MSG "%s runs with the final variant (continuous angles), limited or full, extended_state, and a leaky-relu / relu network of hidden width <= 80"
static int launch_closed_loop(dpenv_handle h, StepArgs& a, PolicyArgs& pa, const IntegArgs* ia, const FilterArgs* fa, hipStream_t s)
{
    const int mode = h->mode, ext = h->cfg.extended_state, ka = pa.ks + 16 * pa.act;
    if (ia && !integ_one_wave(mode, ext, ka))
        return fail(h, DPENV_EINVAL, ONE_WAVE_SET_MSG, "the integral action");
    if (fa && !reff_one_wave(mode, ext, ka))
        return fail(h, DPENV_EINVAL, ONE_WAVE_SET_MSG, "the reference filter");
    const bool general = a.rand_tab || a.loss_on != LOSS_NONE || a.cur_nom;       // hull / current re-draws, a thrust loss
    if ((general && !ws_general(mode, ext, ka)) || (ia && !ws_integ(mode, ext, ka)) || (fa && !ws_reff(mode, ext, ka))) pa.ws = 0;
    hipError_t e;
    if (!pa.ws) {
        bind_shared_loss_as_table(h, a);
        e = pa.split ? dev::launch_policy_rollout_x(&a, &pa, ia, fa, mode, ext, s) : dev::launch_policy_rollout(&a, &pa, ia, fa, mode, ext, s);
    } else if (!pa.split) {
        e = dev::launch_policy_rollout_ws<PREC_F16>(&a, &pa, ia, fa, mode, ext, s);
    } else {
        e = pa.critic_f16 ? dev::launch_policy_rollout_ws<PREC_F32_ACTOR>(&a, &pa, ia, fa, mode, ext, s)
                          : dev::launch_policy_rollout_ws<PREC_F32>(&a, &pa, ia, fa, mode, ext, s);
    }
    if (e != hipSuccess) return fail(h, DPENV_EHIP, "closed-loop launch failed: %s", hipGetErrorString(e));
    return DPENV_OK;
}

static int policy_rollout_impl(dpenv_handle h, const dpenv_policy_rollout_io* io, float* integ_out, float* ref_out, dpenv_stream s)
{
    DeviceGuard dev_guard(h->device);
    if (!h->has_policy) return fail(h, DPENV_EINVAL, "dpenv_set_policy has not been called");
    if (!io || io->struct_size != sizeof(dpenv_policy_rollout_io)) return fail(h, DPENV_EINVAL, "dpenv_policy_rollout_io ABI mismatch");
    if (io->T <= 0 || !io->obs || !io->act || !io->reward || !io->value || !io->logp || !io->done || !io->boot ||
        !io->last_obs || !io->last_value)
        return fail(h, DPENV_EINVAL, "T > 0 and every output block are required");
    if (h->cfg.action_layout != DPENV_AOS || h->cfg.obs_layout != DPENV_AOS)
        return fail(h, DPENV_EINVAL, "policy rollout needs AOS layouts");
    if (int rc = require_classes(h)) return rc;
    if (int rc = check_schedule(h, io)) return rc;
    StepArgs a = h->args;
    bind_optional(h, a, (hipStream_t)s);
    PolicyArgs pa = h->pol;
    pa.T = io->T; pa.noise = io->noise; pa.obs_out = io->obs; pa.act_out = io->act; pa.rew = io->reward; pa.val = io->value;
    pa.logp = io->logp; pa.done = io->done; pa.boot = io->boot; pa.last_obs = io->last_obs; pa.last_val = io->last_value;
    pa.sample = io->sample ? 1 : 0;
    pa.reset_at_end = io->reset_at_end ? 1 : 0;
    pa.use_lag = h->lag_valid ? 1 : 0;
    if (pa.reset_at_end && !h->cfg.auto_reset)
        return fail(h, DPENV_EINVAL, "reset_at_end re-draws every env with the training sampler: it needs config.auto_reset");
    copy_schedule(io, pa);
    IntegArgs ia = h->integ;
    ia.out = integ_out;
    FilterArgs fa = h->reff;
    fa.out = ref_out;
    const int rc = launch_closed_loop(h, a, pa, h->integ_on ? &ia : nullptr, h->reff_on ? &fa : nullptr, (hipStream_t)s);
    if (rc != DPENV_OK) return rc;
    h->lag_valid = true;
    return mark_policy_read(h, s);
}

extern "C" int dpenv_policy_rollout(dpenv_handle h, const dpenv_policy_rollout_io* io, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    return policy_rollout_impl(h, io, nullptr, nullptr, s);
}

extern "C" int dpenv_policy_rollout_integral(dpenv_handle h, const dpenv_policy_rollout_io* io, float* integ_out, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->integ_on) return fail(h, DPENV_EINVAL, "dpenv_policy_rollout_integral: the integral action is off (dpenv_set_integral_action)");
    return policy_rollout_impl(h, io, integ_out, nullptr, s);
}

extern "C" int dpenv_policy_rollout_deployed(dpenv_handle h, const dpenv_policy_rollout_io* io, float* ref_out, float* integ_out, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->reff_on) return fail(h, DPENV_EINVAL, "dpenv_policy_rollout_deployed: the reference filter is off (dpenv_set_reference_filter)");
    if (integ_out && !h->integ_on)
        return fail(h, DPENV_EINVAL, "dpenv_policy_rollout_deployed: integ_out needs the integral action on (dpenv_set_integral_action)");
    return policy_rollout_impl(h, io, integ_out, ref_out, s);
}

// ---- the setpoint reference filter (dpenv.h) -------------------------------------------------------------------------------------
extern "C" int dpenv_set_reference_filter(dpenv_handle h, const dpenv_reference_filter* rf, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!rf) {
        h->reff_on = false;
        return DPENV_OK;
    }
    if (!((h->mode == MODE_FINAL_CONT || h->mode == MODE_LIMITED || h->mode == MODE_FULL) && h->cfg.extended_state))
        return fail(h, DPENV_EINVAL, ONE_WAVE_SET_MSG, "the reference filter");
    FilterArgs& f = h->reff;
    float phi[3][9], gam[3][3];
    if (const char* why = reff_coeffs_f32(rf, h->cfg.substep_dt * (float)h->cfg.n_substeps, phi, gam)) return fail(h, DPENV_EINVAL, "%s", why);
    DeviceGuard dev_guard(h->device);
    if (int rc = ensure_block(h, &f.state, env_bytes(h, 3 * sizeof(float4)), "hipMalloc of the reference filter state failed")) return rc;
    std::memcpy(f.phi, phi, sizeof phi);
    std::memcpy(f.gam, gam, sizeof gam);
    f.out = nullptr;
    HIP_TRY(h, dev::launch_reff_rest(h->args.RF, f.state, nullptr, h->cfg.n_envs, (hipStream_t)s));
    h->reff_on = true;
    return DPENV_OK;
}

extern "C" int dpenv_get_reference_filter_state(dpenv_handle h, float* x_out, float* r_out, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->reff_on) return fail(h, DPENV_EINVAL, "dpenv_get_reference_filter_state: the reference filter is off");
    if (!x_out && !r_out) return fail(h, DPENV_EINVAL, "dpenv_get_reference_filter_state: NULL argument");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_reff_state_io(h->reff.state, x_out, r_out, h->cfg.n_envs, 0, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_set_reference_filter_state(dpenv_handle h, const float* x_in, const float* r_in, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->reff_on) return fail(h, DPENV_EINVAL, "dpenv_set_reference_filter_state: the reference filter is off");
    if (!x_in && !r_in) return fail(h, DPENV_EINVAL, "dpenv_set_reference_filter_state: NULL argument");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_reff_state_io(h->reff.state, (float*)x_in, (float*)r_in, h->cfg.n_envs, 1, (hipStream_t)s));
    return DPENV_OK;
}

// ---- the deployed node's integral action (dpenv.h) -------------------------------------------------------------------------------
extern "C" int dpenv_set_integral_action(dpenv_handle h, const dpenv_integral_action* ia, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!ia) {
        h->integ_on = false;
        return DPENV_OK;
    }
    if (ia->struct_size != sizeof(dpenv_integral_action)) return fail(h, DPENV_EINVAL, "dpenv_integral_action ABI mismatch");
    if (h->mode == MODE_SIMPLE)
        return fail(h, DPENV_EINVAL, "the integral action is not defined for the simple variant (the RL node refuses it, rl_allocator.py:126)");
    for (int j = 0; j < 3; ++j) {
        if (!std::isfinite(ia->gain[j])) return fail(h, DPENV_EINVAL, "integral action: gain[%d] must be finite", j);
        if (std::isnan(ia->bound[j]) || ia->bound[j] < 0.0f) return fail(h, DPENV_EINVAL, "integral action: bound[%d] must be >= 0", j);
        if (std::isnan(ia->box[j]) || ia->box[j] < 0.0f) return fail(h, DPENV_EINVAL, "integral action: box[%d] must be >= 0", j);
    }
    if (!std::isfinite(ia->dwell_s) || ia->dwell_s < 0.0f) return fail(h, DPENV_EINVAL, "integral action: dwell_s must be finite and >= 0");
    if (!std::isfinite(ia->step_s)) return fail(h, DPENV_EINVAL, "integral action: step_s must be finite (<= 0: the control period)");
    // D: the smallest count with D * dt > dwell_s, in f64 (the node's (now - time_arrival) > dwell test in control steps)
    const double dt = (double)h->cfg.substep_dt * (double)h->cfg.n_substeps;
    const double q = (double)ia->dwell_s / dt;
    if (q > 1e9) return fail(h, DPENV_EINVAL, "integral action: dwell_s is more than 1e9 control periods");
    int64_t D = (int64_t)std::floor(q);
    while (D > 0 && (double)(D - 1) * dt > (double)ia->dwell_s) --D;
    while (!((double)D * dt > (double)ia->dwell_s)) ++D;
    DeviceGuard dev_guard(h->device);
    if (int rc = ensure_block(h, &h->integ.state, env_bytes(h, sizeof(float4)), "hipMalloc of the integral state failed")) return rc;
    IntegArgs& g = h->integ;
    for (int j = 0; j < 3; ++j) { g.gain[j] = ia->gain[j]; g.bound[j] = ia->bound[j]; g.box[j] = ia->box[j]; }
    g.step_s = ia->step_s > 0.0f ? ia->step_s : h->cfg.substep_dt * (float)h->cfg.n_substeps;
    g.dwell = (int32_t)D;
    g.out = nullptr;
    HIP_TRY(h, dev::launch_integ_clear(g.state, nullptr, h->cfg.n_envs, (hipStream_t)s));
    h->integ_on = true;
    return DPENV_OK;
}

extern "C" int dpenv_get_integral_state(dpenv_handle h, float* I_out, int32_t* count_out, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->integ_on) return fail(h, DPENV_EINVAL, "dpenv_get_integral_state: the integral action is off");
    if (!I_out && !count_out) return fail(h, DPENV_EINVAL, "dpenv_get_integral_state: NULL argument");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_integ_state_io(h->integ.state, I_out, count_out, h->cfg.n_envs, 0, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_set_integral_state(dpenv_handle h, const float* I_in, const int32_t* count_in, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->integ_on) return fail(h, DPENV_EINVAL, "dpenv_set_integral_state: the integral action is off");
    if (!I_in && !count_in) return fail(h, DPENV_EINVAL, "dpenv_set_integral_state: NULL argument");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_integ_state_io(h->integ.state, (float*)I_in, (int32_t*)count_in, h->cfg.n_envs, 1, (hipStream_t)s));
    return DPENV_OK;
}

#define CONTROL_SET_MSG                                                                                                              \
    "the DP controller runs with the final variant (continuous angles), extended_state, AOS action and observation rows, one vessel " \
    "class (the shared hull, the thrust-loss preset or per-env hulls) and the integral action off"
static bool control_config_ok(dpenv_handle h)
{
    return control_has(h->mode, h->cfg.extended_state != 0) && h->cfg.action_layout == DPENV_AOS && h->cfg.obs_layout == DPENV_AOS &&
           h->n_classes == 1 && !h->integ_on;
}

// back to the pseudo-inverse: a QP allocator, scalar or per-env (the held scalar numbers included), and a neural allocator are dropped
static void allocator_off(dpenv_handle h) { h->stage = ALLOC_PINV; h->qp_scalar = false; h->nn_pop.K = 0; }

extern "C" int dpenv_set_dp_controller(dpenv_handle h, const dpenv_dp_controller* c, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!c) {
        h->ctrl_on = h->ctrl_tab_on = false;
        allocator_off(h);
        return DPENV_OK;
    }
    ControlArgs g = {};
    if (const char* why = control_check(c, g)) return fail(h, DPENV_EINVAL, "%s", why);
    if (!control_config_ok(h)) return fail(h, DPENV_EINVAL, "dpenv_set_dp_controller: " CONTROL_SET_MSG);
    DeviceGuard dev_guard(h->device);
    if (int rc = ensure_block(h, &h->ctrl.z, env_bytes(h, sizeof(float4)), "hipMalloc of the DP controller state failed")) return rc;
    HIP_TRY(h, dev::launch_control_state(h->ctrl.z, nullptr, nullptr, h->cfg.n_envs, 2, (hipStream_t)s));   // (the block stays if this fails)
    g.z = h->ctrl.z;
    g.dt = h->cfg.substep_dt * (float)h->cfg.n_substeps;
    h->ctrl = g;
    h->ctrl_on = true;
    h->ctrl_tab_on = false;                                // the scalar law again: a table in force is dropped
    allocator_off(h);                                      // ... and so is a QP or a neural allocator: the pseudo-inverse allocates again
    return DPENV_OK;
}

#define NN_SET_MSG                                                                                                                   \
    "the NN allocator runs with the DP controller on and its scalar numbers (no per-env controller table in force) and no QP "       \
    "allocator, scalar or per-env, set; while one is set, the controller table and the QP allocator are refused"
#define QP_SET_MSG                                                                                                                   \
    "the QP allocator runs with the DP controller on and its scalar numbers (no per-env controller table), on the shared hull or the " \
    "thrust-loss preset (no per-env hull blocks, one vessel class)"

static_assert(CTRL_NPARAM == DPENV_CTRL_NPARAM && CTRL_KP == DPENV_CTRL_KP && CTRL_KD == DPENV_CTRL_KD && CTRL_KI == DPENV_CTRL_KI &&
                  CTRL_ZB == DPENV_CTRL_ZB && CTRL_TMAX == DPENV_CTRL_TMAX && CTRL_WEIGHT == DPENV_CTRL_WEIGHT && CTRL_LX == DPENV_CTRL_LX &&
                  CTRL_LY == DPENV_CTRL_LY && CTRL_KF == DPENV_CTRL_KF && CTRL_KR_BOW == DPENV_CTRL_KR_BOW && CTRL_F_EPS == DPENV_CTRL_F_EPS,
              "the packing kernel's slots are the header's");

// The rules between the allocation stages, once: may `want` allocate on this handle as it stands - for ALLOC_PINV: from a per-env controller
// table?  NULL, or the refusal's text for behind "<caller>: ".  The setters ask before they change anything; dpenv_controller_rollout asks
// again for the stage in force (the hull kind may have changed since the setter).  Where two rules refuse, the first one listed speaks.
static const char* stage_refusal(dpenv_handle h, int want)
{
    switch (want) {
    case ALLOC_PINV:                                       // (with a controller table: without one nothing stands against it)
        if (qp_flies(h)) return QP_SET_MSG;
        if (h->stage == ALLOC_NN) return "a neural allocator is set: " NN_SET_MSG;
        return nullptr;
    case ALLOC_QP: case ALLOC_QP_TAB:
        if (h->stage == ALLOC_NN) return "a neural allocator is set: " NN_SET_MSG;
        if (h->ctrl_tab_on || h->per_env) return QP_SET_MSG;
        return nullptr;
    default:                                               // ALLOC_NN
        if (h->ctrl_tab_on) return "a per-env controller table is in force: " NN_SET_MSG;
        if (qp_flies(h)) return "a QP allocator is set: " NN_SET_MSG;
        return nullptr;
    }
}

extern "C" int dpenv_set_dp_controller_table(dpenv_handle h, const float* table, uint8_t* refused_out, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->ctrl_on) return fail(h, DPENV_EINVAL, "dpenv_set_dp_controller_table: the DP controller is off (dpenv_set_dp_controller first)");
    if (!table) {
        h->ctrl_tab_on = false;
        return DPENV_OK;
    }
    if (const char* no = stage_refusal(h, ALLOC_PINV)) return fail(h, DPENV_EINVAL, "dpenv_set_dp_controller_table: %s", no);
    DeviceGuard dev_guard(h->device);
    if (int rc = ensure_block(h, &h->ctrl_tab, sizeof(float4) * (size_t)ctrl_tab_float4s(h->cfg.n_envs),     // (whole waves of 64 envs)
                              "hipMalloc of the DP controller table failed")) return rc;
    HIP_TRY(h, dev::launch_pack_controllers(table, h->ctrl_tab, refused_out, h->cfg.n_envs, (hipStream_t)s));
    h->ctrl_tab_on = true;
    return DPENV_OK;
}

extern "C" int dpenv_get_dp_controller_state(dpenv_handle h, float* z_out, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->ctrl_on) return fail(h, DPENV_EINVAL, "dpenv_get_dp_controller_state: the DP controller is off");
    if (!z_out) return fail(h, DPENV_EINVAL, "dpenv_get_dp_controller_state: NULL argument");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_control_state(h->ctrl.z, z_out, nullptr, h->cfg.n_envs, 0, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_set_dp_controller_state(dpenv_handle h, const float* z_in, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!h->ctrl_on) return fail(h, DPENV_EINVAL, "dpenv_set_dp_controller_state: the DP controller is off");
    if (!z_in) return fail(h, DPENV_EINVAL, "dpenv_set_dp_controller_state: NULL argument");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_control_state(h->ctrl.z, (float*)z_in, nullptr, h->cfg.n_envs, 1, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_controller_rollout(dpenv_handle h, const dpenv_controller_rollout_io* io, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (!h->ctrl_on) return fail(h, DPENV_EINVAL, "dpenv_controller_rollout: the DP controller is off (dpenv_set_dp_controller)");
    if (!io || io->struct_size != sizeof(dpenv_controller_rollout_io)) return fail(h, DPENV_EINVAL, "dpenv_controller_rollout_io ABI mismatch");
    if (!control_config_ok(h)) return fail(h, DPENV_EINVAL, "dpenv_controller_rollout: " CONTROL_SET_MSG);
    if (io->T <= 0 || !io->obs || !io->act || !io->reward || !io->done || !io->last_obs)
        return fail(h, DPENV_EINVAL, "T > 0 and the obs, act, reward, done and last_obs blocks are required");
    if (io->ref_out && !h->reff_on)
        return fail(h, DPENV_EINVAL, "dpenv_controller_rollout: ref_out needs the reference filter on (dpenv_set_reference_filter)");
    if (int rc = check_schedule(h, io)) return rc;
    StepArgs a = h->args;
    bind_optional(h, a, (hipStream_t)s);
    ControlArgs ca = h->ctrl;
    ca.T = io->T; ca.obs = io->obs; ca.act = io->act; ca.rew = io->reward; ca.done = io->done; ca.last_obs = io->last_obs;
    copy_schedule(io, ca);
    ca.use_lag = h->lag_valid ? 1 : 0;
    FilterArgs fa = h->reff;
    fa.out = io->ref_out;
    const int ves = rollout_ves(vessel_source(h));
    // the handle may have changed since dpenv_set_qp_allocator: per-env hulls (with control_config_ok, the one way ves leaves the shared forms)
    if (const char* no = stage_refusal(h, h->stage)) return fail(h, DPENV_EINVAL, "dpenv_controller_rollout: %s", no);
    const FilterArgs* fp = h->reff_on ? &fa : nullptr;
    hipError_t e;
    if (h->stage == ALLOC_NN && h->nn_pop.K > 0) {         // a population: the wave's network out of K (dpenv_control_nn_pop.hip)
        e = dev::launch_controller_rollout_nn_pop(&a, &ca, fp, &h->nn_pop, ves, (hipStream_t)s);
    } else if (h->stage == ALLOC_NN) {                     // the neural allocation behind the PID lines: its own kernels (dpenv_control_nn.hip)
        e = dev::launch_controller_rollout_nn(&a, &ca, fp, &h->nn, ves, (hipStream_t)s);
    } else {
        QpRollout qr = h->qp;
        if (h->stage == ALLOC_QP_TAB) qr.q.iters = h->qp_tab_iters;     // (of q only iters is read while the table flies)
        e = dev::launch_controller_rollout(&a, &ca, fp, h->ctrl_tab_on ? h->ctrl_tab : nullptr, qp_flies(h) ? &qr : nullptr,
                                           h->stage == ALLOC_QP_TAB ? h->qp_tab : nullptr, ves, (hipStream_t)s);
    }
    if (e != hipSuccess) return fail(h, DPENV_EHIP, "controller launch failed: %s", hipGetErrorString(e));
    h->lag_valid = true;
    return DPENV_OK;
}

// ---- the QP allocation as the closed loop's allocation stage (dpenv.h) ----
// What dpenv_set_qp_allocator and dpenv_set_qp_allocator_table refuse before they look at their numbers ...
static int qp_setter_before(dpenv_handle h, const char* who)
{
    if (!h->ctrl_on) return fail(h, DPENV_EINVAL, "%s: the DP controller is off (dpenv_set_dp_controller first)", who);
    if (h->stage == ALLOC_NN) return fail(h, DPENV_EINVAL, "%s: %s", who, stage_refusal(h, ALLOC_QP));
    return DPENV_OK;
}
// ... and after them: the handle's configuration, the rest of the stage's rules, and the thruster state's block (on the handle's device)
static int qp_setter_after(dpenv_handle h, const char* who)
{
    if (!control_config_ok(h)) return fail(h, DPENV_EINVAL, "%s: " CONTROL_SET_MSG, who);
    if (const char* no = stage_refusal(h, ALLOC_QP)) return fail(h, DPENV_EINVAL, "%s: %s", who, no);
    return ensure_block(h, &h->qp.state, env_bytes(h, 5 * sizeof(float)), "hipMalloc of the QP allocator state failed");
}

extern "C" int dpenv_set_qp_allocator(dpenv_handle h, const dpenv_qp_allocator* q, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!q) {
        if (qp_flies(h)) allocator_off(h);                 // (a neural allocator stays)
        return DPENV_OK;
    }
    if (int rc = qp_setter_before(h, "dpenv_set_qp_allocator")) return rc;
    QpArgs g = {};
    if (const char* why = qp_check(q, h->ctrl.dt, g)) return fail(h, DPENV_EINVAL, "%s", why);
    DeviceGuard dev_guard(h->device);
    if (int rc = qp_setter_after(h, "dpenv_set_qp_allocator")) return rc;
    HIP_TRY(h, dev::launch_qp_state_clear(h->qp.state, nullptr, h->cfg.n_envs, (hipStream_t)s));   // (the block stays if this fails)
    h->qp.q = g;
    h->stage = ALLOC_QP;                                   // the scalar numbers replace a table in force
    h->qp_scalar = true;
    return DPENV_OK;
}

static_assert(QP_NPARAM == DPENV_QP_NPARAM && QP_WSLACK == DPENV_QP_WSLACK && QP_WPOWER == DPENV_QP_WPOWER && QP_WDALPHA == DPENV_QP_WDALPHA &&
                  QP_WDFORCE == DPENV_QP_WDFORCE && QP_FMAX == DPENV_QP_FMAX && QP_FRATE == DPENV_QP_FRATE && QP_ARATE == DPENV_QP_ARATE &&
                  QP_LX == DPENV_QP_LX && QP_LY == DPENV_QP_LY && QP_KF == DPENV_QP_KF && QP_KR == DPENV_QP_KR,
              "the QP packing kernel's slots are the header's");

// dpenv_set_qp_allocator with row i of the table on env i
extern "C" int dpenv_set_qp_allocator_table(dpenv_handle h, const float* table, int32_t iterations, uint8_t* refused_out, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!table) {                                          // back to the scalar numbers last set, or to the pseudo-inverse; z and x stay
        if (h->stage == ALLOC_QP_TAB) h->stage = h->qp_scalar ? ALLOC_QP : ALLOC_PINV;
        return DPENV_OK;
    }
    if (int rc = qp_setter_before(h, "dpenv_set_qp_allocator_table")) return rc;
    if (iterations < 1 || iterations > QP_MAX_ITERS) return fail(h, DPENV_EINVAL, "QP allocator: iterations must be in 1..32");
    if (!std::isfinite(h->ctrl.dt) || !(h->ctrl.dt > 0.0f)) return fail(h, DPENV_EINVAL, "QP allocator: dt must be finite and > 0");
    DeviceGuard dev_guard(h->device);
    if (int rc = qp_setter_after(h, "dpenv_set_qp_allocator_table")) return rc;
    if (int rc = ensure_block(h, &h->qp_tab, sizeof(float4) * (size_t)qp_tab_float4s(h->cfg.n_envs),          // (whole waves of 64 envs)
                              "hipMalloc of the QP allocator table failed")) return rc;
    HIP_TRY(h, dev::launch_pack_qp_table(table, h->qp_tab, refused_out, h->ctrl.dt, h->cfg.n_envs, (hipStream_t)s));
    HIP_TRY(h, dev::launch_qp_state_clear(h->qp.state, nullptr, h->cfg.n_envs, (hipStream_t)s));
    h->qp_tab_iters = iterations;
    h->stage = ALLOC_QP_TAB;                               // (the scalar numbers, if any are held, stay held)
    return DPENV_OK;
}

// ---- the neural allocation as the closed loop's allocation stage (dpenv.h) ----
// The zero-padded image of K networks of one shape: per layer W [K][in][nn_pad(out)] then b [K][nn_pad(out)], so that network k of a layer
// lies k strides behind network 0 and the kernel needs one product per layer.  A function of the shape and K alone; the one network of
// dpenv_set_nn_allocator is K = 1: per layer W [in][nn_pad(out)] then b [nn_pad(out)].
struct NnImage {
    size_t w_off[NN_MAX_LAYERS], b_off[NN_MAX_LAYERS];     // network 0 of the layer, in floats from the image's base
    size_t floats;
};
static NnImage nn_image_layout(const NnArgs& g, size_t K)
{
    NnImage im = {};
    for (int l = 0; l < g.n_layers; ++l) {
        const size_t in = l == 0 ? g.in_dim : g.H, ld = (size_t)nn_pad(l == g.n_layers - 1 ? 6 : g.H);
        im.w_off[l] = im.floats; im.floats += K * in * ld;
        im.b_off[l] = im.floats; im.floats += K * ld;
    }
    return im;
}

// Writes the image of g's K networks at img (room for nn_image_layout(g, K).floats) and points g's W and b into it.  device: g's arrays are
// DEVICE arrays and one launch packs them; else host arrays: the image is formed here and copied, and the call waits for the copy.
static int nn_install(dpenv_handle h, NnArgs& g, int32_t K, bool device, float* img, dpenv_stream s)
{
    const NnImage im = nn_image_layout(g, (size_t)K);
    if (device) {
        NnPack pk = {};
        pk.n_layers = g.n_layers; pk.in_dim = g.in_dim; pk.H = g.H; pk.K = K;
        for (int l = 0; l < g.n_layers; ++l) {
            pk.W[l] = g.W[l]; pk.b[l] = g.b[l];
            pk.dW[l] = img + im.w_off[l]; pk.db[l] = img + im.b_off[l];
        }
        HIP_TRY(h, dev::launch_nn_pack(&pk, (hipStream_t)s));
    } else {
        std::vector<float> host(im.floats, 0.0f);
        for (int l = 0; l < g.n_layers; ++l) {
            const size_t in = l == 0 ? g.in_dim : g.H, out = l == g.n_layers - 1 ? 6 : g.H, ld = (size_t)nn_pad((int)out);
            float* dW = host.data() + im.w_off[l];
            float* db = host.data() + im.b_off[l];
            for (size_t q = 0; q < (size_t)K; ++q) {
                for (size_t k = 0; k < in; ++k)
                    for (size_t j = 0; j < out; ++j) dW[q * in * ld + k * ld + j] = g.W[l][q * in * out + k * out + j];
                for (size_t j = 0; j < out; ++j) db[q * ld + j] = g.b[l][q * out + j];
            }
        }
        HIP_TRY(h, hipMemcpyAsync(img, host.data(), sizeof(float) * im.floats, hipMemcpyHostToDevice, (hipStream_t)s));
        HIP_TRY(h, hipStreamSynchronize((hipStream_t)s));
    }
    for (int l = 0; l < g.n_layers; ++l) { g.W[l] = img + im.w_off[l]; g.b[l] = img + im.b_off[l]; }
    return DPENV_OK;
}

// What dpenv_set_nn_allocator and dpenv_set_nn_allocator_population do before anything of their own: a NULL `a` turns a neural allocator
// off (a QP allocator stays); else the refusals in their order, `own` (the population's rules about K, envs_per_net and env_id_base; NULL
// or the text for behind "<who>: ") between those about the struct and those about the handle.  NN_SET_GO: go on with g; else the return.
enum { NN_SET_GO = 1 };
template <typename Own>
static int nn_setter_open(dpenv_handle h, const dpenv_nn_allocator* a, const char* who, NnArgs& g, Own&& own)
{
    if (!h) return DPENV_EINVAL;
    if (!a) {
        if (h->stage == ALLOC_NN) allocator_off(h);
        return DPENV_OK;
    }
    if (!h->ctrl_on) return fail(h, DPENV_EINVAL, "%s: the DP controller is off (dpenv_set_dp_controller first)", who);
    if (const char* why = nn_check(a, g)) return fail(h, DPENV_EINVAL, "%s", why);
    if (a->device_pointers != 0 && a->device_pointers != 1) return fail(h, DPENV_EINVAL, "NN allocator: device_pointers must be 0 or 1");
    if (const char* why = own()) return fail(h, DPENV_EINVAL, "%s: %s", who, why);
    if (!control_config_ok(h)) return fail(h, DPENV_EINVAL, "%s: " CONTROL_SET_MSG, who);
    if (const char* no = stage_refusal(h, ALLOC_NN)) return fail(h, DPENV_EINVAL, "%s: %s", who, no);
    return NN_SET_GO;
}

extern "C" int dpenv_set_nn_allocator(dpenv_handle h, const dpenv_nn_allocator* a, dpenv_stream s)
{
    NnArgs g;
    const int open = nn_setter_open(h, a, "dpenv_set_nn_allocator", g, [] { return (const char*)nullptr; });
    if (open != NN_SET_GO) return open;
    DeviceGuard dev_guard(h->device);
    // the largest shape's image, once: a later call never allocates
    if (int rc = ensure_block(h, &h->nn_img, sizeof(float) * (size_t)NN_IMAGE_FLOATS, "hipMalloc of the NN allocator image failed")) return rc;
    if (int rc = nn_install(h, g, 1, a->device_pointers != 0, h->nn_img, s)) return rc;
    h->nn.a = g;
    h->stage = ALLOC_NN;
    h->nn_pop.K = 0;                                       // one network: a population in force is replaced
    return DPENV_OK;
}

// K networks of one shape, one per envs_per_net envs (dpenv.h)
extern "C" int dpenv_set_nn_allocator_population(dpenv_handle h, const dpenv_nn_allocator* a, int32_t K, int32_t envs_per_net, dpenv_stream s)
{
    NnArgs g;
    const int open = nn_setter_open(h, a, "dpenv_set_nn_allocator_population", g, [&]() -> const char* {
        if (const char* why = nn_pop_check(K, envs_per_net)) return why;
        if (h->args.env_id_base < 0 || h->args.env_id_base % RBLOCK != 0)
            return "env_id_base must be >= 0 and a multiple of 64 (a wave must not straddle two networks)";
        return nullptr;
    });
    if (open != NN_SET_GO) return open;
    DeviceGuard dev_guard(h->device);
    const int32_t shape[4] = {g.n_layers, g.in_dim, g.H, K};
    if (!h->nn_pop_img || std::memcmp(shape, h->nn_pop_shape, sizeof shape) != 0) {   // another shape or K: a new image; the old one goes last
        const size_t bytes = sizeof(float) * nn_image_layout(g, (size_t)K).floats;
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, DPENV_ENOMEM, "hipMalloc of the NN allocator population image failed (%zu bytes)", bytes);
        }
        if (h->nn_pop_img) {
            if (h->stage == ALLOC_NN && h->nn_pop.K > 0) allocator_off(h);     // (nothing may fly addresses of the image that goes)
            (void)hipFree(h->nn_pop_img);
        }
        h->nn_pop_img = (float*)p;
        std::memcpy(h->nn_pop_shape, shape, sizeof shape);
    }
    if (int rc = nn_install(h, g, K, a->device_pointers != 0, h->nn_pop_img, s)) return rc;
    const int64_t wpn = envs_per_net / RBLOCK;
    h->nn_pop.a = g;
    h->nn_pop.waves_per_net = (int32_t)wpn;
    h->nn_pop.wave_base = (uint32_t)((h->args.env_id_base / RBLOCK) % (wpn * (int64_t)K));
    h->nn_pop.K = K;
    h->stage = ALLOC_NN;
    return DPENV_OK;
}

// dpenv_get_qp_allocator_state / dpenv_set_qp_allocator_state: one copy with the direction swapped (as current_io)
static int qp_state_io(dpenv_handle h, const char* who, float* theirs, bool set, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    if (!qp_flies(h)) return fail(h, DPENV_EINVAL, "%s: no QP allocator is set", who);
    if (!theirs) return fail(h, DPENV_EINVAL, "%s: NULL argument", who);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, hipMemcpyAsync(set ? h->qp.state : theirs, set ? theirs : h->qp.state, env_bytes(h, 5 * sizeof(float)), hipMemcpyDeviceToDevice, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_get_qp_allocator_state(dpenv_handle h, float* state_out, dpenv_stream s)
{
    return qp_state_io(h, "dpenv_get_qp_allocator_state", state_out, false, s);
}

extern "C" int dpenv_set_qp_allocator_state(dpenv_handle h, const float* state_in, dpenv_stream s)
{
    return qp_state_io(h, "dpenv_set_qp_allocator_state", (float*)state_in, true, s);
}

// the shared opening of the four label entry points (who: the entry point's name, whose io struct is <who>_io); act_optional: the scan
// has another output the caller may want instead, and says itself which of them it needs
template <class IO>
static int check_label_io(dpenv_handle h, const char* who, const IO* io, bool act_optional = false)
{
    if (!h->ctrl_on) return fail(h, DPENV_EINVAL, "%s: the DP controller is off (dpenv_set_dp_controller)", who);
    if (!io || io->struct_size != sizeof(IO)) return fail(h, DPENV_EINVAL, "%s_io ABI mismatch", who);
    if (io->T <= 0) return fail(h, DPENV_EINVAL, "%s: T > 0 is required", who);
    if (act_optional) {
        if (!io->obs) return fail(h, DPENV_EINVAL, "%s: the obs block is required", who);
    } else if (!io->obs || !io->act) return fail(h, DPENV_EINVAL, "%s: the obs and act blocks are required", who);
    if (io->obs_dtype != DPENV_F32 && io->obs_dtype != DPENV_BF16) return fail(h, DPENV_EINVAL, "%s: obs_dtype must be DPENV_F32 or DPENV_BF16", who);
    return DPENV_OK;
}

// the law on rows some other flight wrote: nothing of the handle but the controller's numbers (or its table) and dt is read
extern "C" int dpenv_controller_label(dpenv_handle h, const dpenv_controller_label_io* io, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (int rc = check_label_io(h, "dpenv_controller_label", io)) return rc;
    LabelArgs la = {};
    la.obs = io->obs; la.done = io->done; la.z_in = io->z_in; la.z_out = io->z_out; la.act = io->act;
    la.T = io->T; la.n = h->cfg.n_envs;
    const hipError_t e = dev::launch_controller_label(&h->ctrl, &la, h->ctrl_tab_on ? h->ctrl_tab : nullptr, io->obs_dtype == DPENV_BF16, (hipStream_t)s);
    if (e != hipSuccess) return fail(h, DPENV_EHIP, "label launch failed: %s", hipGetErrorString(e));
    return DPENV_OK;
}

// the scan's argument block of dpenv_controller_label_qp_io and dpenv_controller_label_qp_ex_io
template <class IO>
static LabelQpArgs fill_label_qp_args(const IO* io, int n)
{
    LabelQpArgs la = {};
    la.obs = io->obs; la.done = io->done; la.z_in = io->z_in; la.z_out = io->z_out; la.x_in = io->x_in; la.x_out = io->x_out;
    la.act = io->act; la.cost = io->cost;
    la.T = io->T; la.n = n;
    return la;
}

// which QP numbers a label call without a table of its own scans with: q's, else the ones dpenv_set_qp_allocator has in force.  takes / pass:
// the two calls' wordings of what the scan takes and what the caller can pass instead
static int resolve_label_qp_numbers(dpenv_handle h, const char* who, const dpenv_qp_allocator* q, const char* takes, const char* pass, QpArgs& g)
{
    if (q) {
        if (const char* why = qp_check(q, h->ctrl.dt, g)) return fail(h, DPENV_EINVAL, "%s", why);
    } else if (h->stage == ALLOC_QP_TAB) {
        return fail(h, DPENV_EINVAL, "%s: a per-env QP table (dpenv_set_qp_allocator_table) is in force and the scan takes %s: pass %s", who, takes, pass);
    } else if (h->stage == ALLOC_QP) {
        g = h->qp.q;
    } else {
        return fail(h, DPENV_EINVAL, "%s: no QP allocator (pass %s, or dpenv_set_qp_allocator first)", who, pass);
    }
    return DPENV_OK;
}

// ... with the QP allocation behind the PID lines: io->q's numbers, or the ones dpenv_set_qp_allocator has in force.  The handle's hull
// kind does not matter (no hull is touched), and neither its z nor its QP thruster state is read or written.
extern "C" int dpenv_controller_label_qp(dpenv_handle h, const dpenv_controller_label_qp_io* io, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (int rc = check_label_io(h, "dpenv_controller_label_qp", io)) return rc;
    QpArgs g = {};
    if (int rc = resolve_label_qp_numbers(h, "dpenv_controller_label_qp", io->q, "one set of numbers", "q", g)) return rc;
    const LabelQpArgs la = fill_label_qp_args(io, h->cfg.n_envs);
    const hipError_t e = dev::launch_controller_label_qp(&h->ctrl, &g, &la, h->ctrl_tab_on ? h->ctrl_tab : nullptr, io->obs_dtype == DPENV_BF16,
                                                         (hipStream_t)s);
    if (e != hipSuccess) return fail(h, DPENV_EHIP, "QP label launch failed: %s", hipGetErrorString(e));
    return DPENV_OK;
}

// ... with the thruster state taken from the flown action rows and / or one QP allocator per env, read from the public table by the lanes
// themselves.  With neither, the call above (its kernels, its launcher).
extern "C" int dpenv_controller_label_qp_ex(dpenv_handle h, const dpenv_controller_label_qp_ex_io* io, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (int rc = check_label_io(h, "dpenv_controller_label_qp_ex", io)) return rc;
    if (io->q && io->qp_table) return fail(h, DPENV_EINVAL, "dpenv_controller_label_qp_ex: q or qp_table, not both");
    if (io->refused_out && !io->qp_table) return fail(h, DPENV_EINVAL, "dpenv_controller_label_qp_ex: refused_out goes with qp_table");
    QpArgs g = {};
    if (io->qp_table) {
        if (io->iterations < 1 || io->iterations > QP_MAX_ITERS) return fail(h, DPENV_EINVAL, "QP allocator: iterations must be in 1..32");
        if (!std::isfinite(h->ctrl.dt) || !(h->ctrl.dt > 0.0f)) return fail(h, DPENV_EINVAL, "QP allocator: dt must be finite and > 0");
    } else if (int rc = resolve_label_qp_numbers(h, "dpenv_controller_label_qp_ex", io->q, "the numbers of the call", "q or qp_table", g)) {
        return rc;
    }
    const LabelQpArgs la = fill_label_qp_args(io, h->cfg.n_envs);
    const float4* tab = h->ctrl_tab_on ? h->ctrl_tab : nullptr;
    const int bf16 = io->obs_dtype == DPENV_BF16;
    hipError_t e;
    if (!io->flown && !io->qp_table) {
        e = dev::launch_controller_label_qp(&h->ctrl, &g, &la, tab, bf16, (hipStream_t)s);
    } else {
        LabelQpExArgs xa = {};
        xa.flown = io->flown; xa.qp_table = io->qp_table; xa.refused = io->refused_out; xa.iters = io->iterations;
        e = dev::launch_controller_label_qp_ex(&h->ctrl, &g, &la, &xa, tab, bf16, (hipStream_t)s);
    }
    if (e != hipSuccess) return fail(h, DPENV_EHIP, "QP label launch failed: %s", hipGetErrorString(e));
    return DPENV_OK;
}

// ... with the neural allocation behind the PID lines and / or the PID's wrench per row: io->a's network read in place, or the image and
// constants dpenv_set_nn_allocator has in force.  Of the handle only the controller's numbers (or its table), dt and that image are read.
extern "C" int dpenv_controller_label_nn(dpenv_handle h, const dpenv_controller_label_nn_io* io, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    if (int rc = check_label_io(h, "dpenv_controller_label_nn", io, true)) return rc;
    if (!io->act && !io->tau_out) return fail(h, DPENV_EINVAL, "dpenv_controller_label_nn: act and tau_out are both NULL (nothing to write)");
    if (io->raw && !io->act) return fail(h, DPENV_EINVAL, "dpenv_controller_label_nn: raw goes with act");
    NnArgs g = {};
    const bool own = io->a != nullptr;
    if (io->act) {                                         // (the wrench-only scan does not look at a)
        if (own) {
            if (const char* why = nn_check_in_place(io->a, g)) return fail(h, DPENV_EINVAL, "%s", why);
        } else if (h->stage == ALLOC_NN && h->nn_pop.K > 0) {
            return fail(h, DPENV_EINVAL, "dpenv_controller_label_nn: a population of networks is in force and the scan takes one network (pass a)");
        } else if (h->stage == ALLOC_NN) {
            g = h->nn.a;
        } else {
            return fail(h, DPENV_EINVAL, "dpenv_controller_label_nn: no neural allocator (pass a, or dpenv_set_nn_allocator first)");
        }
    }
    LabelNnArgs la = {};
    la.obs = io->obs; la.done = io->done; la.z_in = io->z_in; la.z_out = io->z_out;
    la.act = io->act; la.raw = io->raw; la.tau = io->tau_out;
    la.T = io->T; la.n = h->cfg.n_envs;
    const hipError_t e = dev::launch_controller_label_nn(&h->ctrl, io->act ? &g : nullptr, &la, h->ctrl_tab_on ? h->ctrl_tab : nullptr,
                                                         io->obs_dtype == DPENV_BF16, own ? 0 : 1, (hipStream_t)s);
    if (e != hipSuccess) return fail(h, DPENV_EHIP, "NN label launch failed: %s", hipGetErrorString(e));
    return DPENV_OK;
}

extern "C" int dpenv_get_state(dpenv_handle h, float* state_out, int32_t* counters_out, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_get_state(&h->args, state_out, counters_out, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_set_state(dpenv_handle h, const float* state_in, const int32_t* counters_in, dpenv_stream s)
{
    if (!h) return DPENV_EINVAL;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev::launch_set_state(&h->args, state_in, counters_in, (hipStream_t)s));
    if (state_in) h->lag_valid = true;                     // the kernel wrote the columns a state-rebuilt observation carries (pt / 100)
    return DPENV_OK;
}

// exploration-noise and current-drift draw counters: with them a restored state reproduces sampled rollouts (dpenv.h)
extern "C" int dpenv_get_rng_counters(dpenv_handle h, uint32_t* noise_ctr_out, uint32_t* drift_ctr_out, dpenv_stream s)
{
    if (!h || (!noise_ctr_out && !drift_ctr_out)) return fail(h, DPENV_EINVAL, "dpenv_get_rng_counters: NULL argument");
    DeviceGuard dev_guard(h->device);
    const size_t bytes = sizeof(uint32_t) * (size_t)h->cfg.n_envs;
    if (noise_ctr_out) HIP_TRY(h, hipMemcpyAsync(noise_ctr_out, h->noise_ctr, bytes, hipMemcpyDeviceToDevice, (hipStream_t)s));
    if (drift_ctr_out) HIP_TRY(h, hipMemcpyAsync(drift_ctr_out, h->drift_ctr, bytes, hipMemcpyDeviceToDevice, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_set_rng_counters(dpenv_handle h, const uint32_t* noise_ctr_in, const uint32_t* drift_ctr_in, dpenv_stream s)
{
    if (!h || (!noise_ctr_in && !drift_ctr_in)) return fail(h, DPENV_EINVAL, "dpenv_set_rng_counters: NULL argument");
    DeviceGuard dev_guard(h->device);
    const size_t bytes = sizeof(uint32_t) * (size_t)h->cfg.n_envs;
    if (noise_ctr_in) HIP_TRY(h, hipMemcpyAsync(h->noise_ctr, noise_ctr_in, bytes, hipMemcpyDeviceToDevice, (hipStream_t)s));
    if (drift_ctr_in) HIP_TRY(h, hipMemcpyAsync(h->drift_ctr, drift_ctr_in, bytes, hipMemcpyDeviceToDevice, (hipStream_t)s));
    return DPENV_OK;
}

// the thrust columns of the observation the last closed-loop launch ended with (PolicyArgs.use_lag): part of a mid-episode checkpoint
extern "C" int dpenv_get_obs_thrust(dpenv_handle h, float* out, dpenv_stream s)
{
    if (!h || !out) return fail(h, DPENV_EINVAL, "dpenv_get_obs_thrust: NULL argument");
    if (!h->lag_valid) return fail(h, DPENV_EINVAL, "the lagged thrust columns are stale (dpenv_step ran without a policy in force, or a masked reset on stale columns): the next closed-loop launch starts from the state block alone");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, hipMemcpyAsync(out, h->args.S3, sizeof(float4) * (size_t)h->cfg.n_envs, hipMemcpyDeviceToDevice, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_set_obs_thrust(dpenv_handle h, const float* in, dpenv_stream s)
{
    if (!h || !in) return fail(h, DPENV_EINVAL, "dpenv_set_obs_thrust: NULL argument");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, hipMemcpyAsync(h->args.S3, in, sizeof(float4) * (size_t)h->cfg.n_envs, hipMemcpyDeviceToDevice, (hipStream_t)s));
    h->lag_valid = true;
    return DPENV_OK;
}

