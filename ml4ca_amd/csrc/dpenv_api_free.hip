// dpenv_api_free.hip - the entry points of the C ABI (include/dpenv.h) that take no handle: the defaults, the stateless device helpers
// (thrust map, allocation, GAE, advantage statistics, score card, the PPO update) and the pure validators they share with the handle code in
// dpenv_api.hip (dpenv_host.h).  Nothing here can look inside a handle: its struct is private to dpenv_api.hip.
#include <cmath>
#include <cstring>
#include <string>

#include "dpenv_host.h"
#include "dpenv_train_dev.h"

using namespace dpenv;
using namespace dpenv::host;

extern "C" int dpenv_abi_version(void) { return DPENV_ABI_VERSION; }

extern "C" int dpenv_default_config(dpenv_config* c)
{
    if (!c) return DPENV_EINVAL;
    std::memset(c, 0, sizeof *c);
    c->struct_size = (uint32_t)sizeof *c;
    c->n_envs = 0;
    c->device = -1;
    c->variant = DPENV_FINAL;      // train.py:47 'final'
    c->extended_state = 1;         // train.py:52
    c->cont_ang = 1;               // train.py:54
    c->n_substeps = 20;            // customEnv.py:79-80
    c->substep_dt = 0.01f;         // customEnv.py:81
    c->wrap_mode = DPENV_WRAP_REFERENCE;
    c->terminate = 1;
    c->max_ep_len = 400;           // customEnv.py:83 with max_ep_len=800, n_steps=20
    c->auto_reset = 0;
    c->action_layout = DPENV_AOS;
    c->obs_layout = DPENV_AOS;
    c->obs_dtype = DPENV_F32;
    c->current_enabled = 0;
    c->seed = 0;
    c->env_id_base = 0;
    c->reset_fraction = 0.8f;      // customEnv.py:135
    c->current_drift = 0;
    c->current_tau = 100.0f;                           // SURVEY 8(d) config 5 (build-defined)
    c->current_sigma_v = 0.02f;
    c->current_sigma_beta = 5.0f * 3.14159265358979f / 180.0f;
    c->reset_acts = 0;             // customEnv.py:30 reset_acts=False
    return DPENV_OK;
}

// BUILD-OWNED hull + the reference's thruster constants
// (qp_allocator.py:51-55 K "as currently set in the simulator", :69-70 lever arms; env order bow,port,star).
extern "C" int dpenv_default_vessel(float* p)
{
    if (!p) return DPENV_EINVAL;
    for (int i = 0; i < DPENV_NPARAM; ++i) p[i] = 0.0f;
    // fitted to the reference's recorded Cybersea runs by tests/calibration/calibrate_plant.py
    p[DPENV_P_M11] = 263.93f; p[DPENV_P_M22] = 300.9f; p[DPENV_P_M23] = 7.0f; p[DPENV_P_M33] = 300.0f;
    p[DPENV_P_XU] = 3.0f;  p[DPENV_P_XUU] = 7.1f;
    p[DPENV_P_YV] = 19.8f; p[DPENV_P_YVV] = 80.3f;
    p[DPENV_P_YR] = -1.1f; p[DPENV_P_NV] = 19.7f;
    p[DPENV_P_NR] = 77.8f; p[DPENV_P_NRR] = 24.9f;
    p[DPENV_P_NUV] = 40.0f; p[DPENV_P_YUR] = 30.0f;
    p[DPENV_P_KF_BOW] = 0.0009f; p[DPENV_P_KF_PORT] = 0.00205f; p[DPENV_P_KF_STAR] = 0.00205f;
    p[DPENV_P_KR_BOW] = 0.0009f; p[DPENV_P_KR_PORT] = 0.00205f; p[DPENV_P_KR_STAR] = 0.00205f;
    p[DPENV_P_LX_BOW] = 1.08f; p[DPENV_P_LX_PORT] = -1.12f; p[DPENV_P_LX_STAR] = -1.12f;
    p[DPENV_P_LY_BOW] = 0.0f;  p[DPENV_P_LY_PORT] = -0.15f; p[DPENV_P_LY_STAR] = 0.15f;
    return DPENV_OK;
}

// The same hull with the thrust gains of the reference's SECOND set of steady full-thrust speeds - "with thrust losses" +1.4 / -1.1 m/s
// ahead / astern (customEnv.py:17), which are also the velocity bounds it trains with (customEnv.py:26) - derived by
// tests/calibration/fit_thrust_loss_preset.py as an INFLOW loss of the stern thrusters, F = K n|n| - Kl |n| u_a (u_a: the water's speed
// along the thruster axis; never past zero thrust), their reverse gain from the no-loss astern speed (-1.60 m/s, customEnv.py:14); bow
// unchanged (sway 0.29 m/s against the recorded 0.30); the hull is untouched, so the free-drift record is reproduced as before.  Yaw comes
// out at 0.505 rad/s against the recorded 0.52 (a constant gain reduced to meet +1.4 m/s - round 5's first form of this preset - gave 0.35).
// Not the default: the loss code lives in the general per-env kernels only (DESIGN.md section 3 for what it costs and what it changes).
extern "C" int dpenv_default_vessel_ex(int32_t kind, float* p)
{
    if (!p || kind < 0 || kind > (DPENV_VESSEL_THRUST_LOSS | DPENV_VESSEL_DYNPOS_FIT)) return DPENV_EINVAL;
    dpenv_default_vessel(p);
    if (kind & DPENV_VESSEL_DYNPOS_FIT) {
        // tests/calibration/fit_dynpos_preset.py (round 6): the sway-yaw part of the hull refitted JOINTLY to what the default is fitted to (free
        // drift, box test, steady surge / yaw speeds) AND to the reference's 32 recorded station-keeping runs in a current from 16 directions
        // (results/all_plots/dyn_pos/) AND to the recorded steady sway speed 0.35 m/s (customEnv.py:14), which the default hull misses (0.29)
        p[DPENV_P_M22] = 317.3f; p[DPENV_P_M33] = 300.0f;
        p[DPENV_P_YV] = 21.4f; p[DPENV_P_YVV] = 54.3f; p[DPENV_P_YR] = -4.9f;
        p[DPENV_P_NV] = 11.4f; p[DPENV_P_NR] = 57.0f; p[DPENV_P_NRR] = 59.6f;
        p[DPENV_P_NUV] = 40.0f; p[DPENV_P_YUR] = 25.3f;
    }
    if (kind & DPENV_VESSEL_THRUST_LOSS) {
        // tests/calibration/fit_thrust_loss_preset.py: stern reverse gain from -1.60 m/s astern without losses, inflow-loss coefficients from
        // +1.4 / -1.1 m/s with losses (customEnv.py:14,17); the bow thruster keeps its gain and has no loss.  (Surge only: the same numbers on
        // either hull - Xu, Xuu and m11 are not part of the dyn_pos fit.)
        p[DPENV_P_KR_PORT] = p[DPENV_P_KR_STAR] = 0.001149f;
        p[DPENV_P_KLF_PORT] = p[DPENV_P_KLF_STAR] = 0.08173f;
        p[DPENV_P_KLR_PORT] = p[DPENV_P_KLR_STAR] = 0.05039f;
    }
    return DPENV_OK;
}

int host::mode_of(const dpenv_config* c)
{
    switch (c->variant) {
    case DPENV_FULL: return MODE_FULL;
    case DPENV_SIMPLE: return MODE_SIMPLE;
    case DPENV_LIMITED: return MODE_LIMITED;
    case DPENV_FINAL: return c->cont_ang ? MODE_FINAL_CONT : MODE_FINAL_WRAP;
    }
    return -1;
}

extern "C" int dpenv_act_dim(const dpenv_config* c)
{
    if (!c) return DPENV_EINVAL;
    switch (mode_of(c)) {
    case MODE_FULL: return 6;          // customEnv.py:24
    case MODE_SIMPLE: return 3;        // :332
    case MODE_LIMITED: return 5;       // :356
    case MODE_FINAL_WRAP: return 5;    // :379
    case MODE_FINAL_CONT: return 7;
    }
    return DPENV_EINVAL;
}

extern "C" int dpenv_obs_dim(const dpenv_config* c)
{
    if (!c) return DPENV_EINVAL;
    return c->extended_state ? 9 : 6;   // customEnv.py:44
}

int host::derive_vessel(const float* p, VesselDev* d, std::string* why, bool allow_loss)
{
    const double m11 = p[DPENV_P_M11], m22 = p[DPENV_P_M22], m23 = p[DPENV_P_M23], m33 = p[DPENV_P_M33];
    const double det = m22 * m33 - m23 * m23;
    if (!(m11 > 0.0) || !(det > 0.0) || !(m22 > 0.0)) {
        *why = "mass matrix is not positive definite";
        return DPENV_EINVAL;
    }
    for (int i = 0; i < DPENV_NPARAM; ++i)
        if (!std::isfinite(p[i])) { *why = "vessel parameter is not finite"; return DPENV_EINVAL; }
    d->p[VD_M11] = (float)m11; d->p[VD_M22] = (float)m22; d->p[VD_M23] = (float)m23;
    // same float operations as the fp32 oracle so that both sides integrate with identical constants
    const float fm11 = (float)m11, fm22 = (float)m22, fm23 = (float)m23, fm33 = (float)m33;
    const float fdet = fm22 * fm33 - fm23 * fm23;
    d->p[VD_INV11] = 1.0f / fm11;
    d->p[VD_I22] = fm33 / fdet; d->p[VD_I23] = -fm23 / fdet; d->p[VD_I33] = fm22 / fdet;
    d->p[VD_XU] = p[DPENV_P_XU]; d->p[VD_XUU] = p[DPENV_P_XUU]; d->p[VD_YV] = p[DPENV_P_YV];
    d->p[VD_YVV] = p[DPENV_P_YVV]; d->p[VD_YR] = p[DPENV_P_YR]; d->p[VD_NV] = p[DPENV_P_NV];
    d->p[VD_NR] = p[DPENV_P_NR]; d->p[VD_NRR] = p[DPENV_P_NRR];
    d->p[VD_NUV] = p[DPENV_P_NUV]; d->p[VD_YUR] = p[DPENV_P_YUR];
    for (int i = 0; i < 3; ++i) {
        d->p[VD_KF + i] = p[DPENV_P_KF_BOW + i]; d->p[VD_KR + i] = p[DPENV_P_KR_BOW + i];
        d->p[VD_LX + i] = p[DPENV_P_LX_BOW + i]; d->p[VD_LY + i] = p[DPENV_P_LY_BOW + i];
        if (!(p[DPENV_P_KLF_BOW + i] >= 0.0f) || !(p[DPENV_P_KLR_BOW + i] >= 0.0f)) { *why = "thrust-loss coefficients must be >= 0"; return DPENV_EINVAL; }
        if (!allow_loss && (p[DPENV_P_KLF_BOW + i] != 0.0f || p[DPENV_P_KLR_BOW + i] != 0.0f)) {
            *why = "thrust-loss coefficients (parameters 26-31) are not available to vessel CLASSES: one class, per-env blocks (dpenv_set_vessel_params) or the nominal hull of dpenv_set_vessel_randomisation";
            return DPENV_EINVAL;
        }
    }
    return DPENV_OK;
}

// ---- the setpoint reference filter's coefficients (dpenv.h) -----------------------------------------------------------------------
// exp(M) of the 4x4 augmented system M = [[A, B], [0, 0]] dt of one axis, in f64: scaling and squaring of the degree-18 Taylor polynomial
// (||M / 2^sq||_1 <= 1/2: truncation below 1e-22).  deploy.reference_filter_coeffs_f64 is the same recipe in NumPy.
static void reff_coeffs_f64(double w, double z, double dt, double phi[9], double gam[3])
{
    const double c = 2.0 * z + 1.0;
    double M[4][4] = {{0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {-w * w * w, -c * w * w, -c * w, w * w * w}, {0.0, 0.0, 0.0, 0.0}};
    double norm = 0.0;
    for (int col = 0; col < 4; ++col) {
        double sum = 0.0;
        for (int r = 0; r < 4; ++r) { M[r][col] *= dt; sum += std::fabs(M[r][col]); }
        norm = std::fmax(norm, sum);
    }
    int sq = 0;
    while (norm > 0.5 && sq < 200) { norm *= 0.5; ++sq; }
    const double scale = std::ldexp(1.0, -sq);
    for (int r = 0; r < 4; ++r) for (int col = 0; col < 4; ++col) M[r][col] *= scale;
    double E[4][4], T[4][4];                                     // E = sum_k M^k / k!, T = the running term
    for (int r = 0; r < 4; ++r) for (int col = 0; col < 4; ++col) E[r][col] = T[r][col] = (r == col) ? 1.0 : 0.0;
    for (int k = 1; k <= 18; ++k) {
        double U[4][4];
        for (int r = 0; r < 4; ++r) for (int col = 0; col < 4; ++col) {
            double acc = 0.0;
            for (int q = 0; q < 4; ++q) acc += T[r][q] * M[q][col];
            U[r][col] = acc / (double)k;
        }
        for (int r = 0; r < 4; ++r) for (int col = 0; col < 4; ++col) { T[r][col] = U[r][col]; E[r][col] += U[r][col]; }
    }
    for (int k = 0; k < sq; ++k) {
        double U[4][4];
        for (int r = 0; r < 4; ++r) for (int col = 0; col < 4; ++col) {
            double acc = 0.0;
            for (int q = 0; q < 4; ++q) acc += E[r][q] * E[q][col];
            U[r][col] = acc;
        }
        std::memcpy(E, U, sizeof E);
    }
    for (int r = 0; r < 3; ++r) {
        for (int col = 0; col < 3; ++col) phi[3 * r + col] = E[r][col];
        gam[r] = E[r][3];
    }
}

static const char* reff_check(const dpenv_reference_filter* rf)
{
    if (rf->struct_size != sizeof(dpenv_reference_filter)) return "dpenv_reference_filter ABI mismatch";
    for (int j = 0; j < 3; ++j) {
        if (!std::isfinite(rf->omega[j]) || !(rf->omega[j] > 0.0f)) return "reference filter: omega must be finite and > 0 on every axis";
        if (!std::isfinite(rf->zeta[j]) || !(rf->zeta[j] > 0.0f)) return "reference filter: zeta must be finite and > 0 on every axis";
    }
    return nullptr;
}

const char* host::reff_coeffs_f32(const dpenv_reference_filter* rf, float dt, float phi[3][9], float gam[3][3])
{
    if (const char* why = reff_check(rf)) return why;
    if (!std::isfinite(dt) || !(dt > 0.0f)) return "reference filter: dt must be finite and > 0";
    for (int j = 0; j < 3; ++j) {
        double p[9], g[3];
        reff_coeffs_f64((double)rf->omega[j], (double)rf->zeta[j], (double)dt, p, g);
        for (int k = 0; k < 9; ++k) phi[j][k] = (float)p[k];
        for (int k = 0; k < 3; ++k) gam[j][k] = (float)g[k];
        for (int k = 0; k < 9; ++k) if (!std::isfinite(phi[j][k])) return "reference filter: omega * dt too large (the coefficients overflow f32)";
        for (int k = 0; k < 3; ++k) if (!std::isfinite(gam[j][k])) return "reference filter: omega * dt too large (the coefficients overflow f32)";
    }
    return nullptr;
}

extern "C" int dpenv_reference_filter_coeffs(const dpenv_reference_filter* rf, float dt, float phi_out[3][9], float gam_out[3][3])
{
    if (!rf || !phi_out || !gam_out) return fail(nullptr, DPENV_EINVAL, "dpenv_reference_filter_coeffs: NULL argument");
    float phi[3][9], gam[3][3];
    if (const char* why = reff_coeffs_f32(rf, dt, phi, gam)) return fail(nullptr, DPENV_EINVAL, "%s", why);
    std::memcpy(phi_out, phi, sizeof phi);
    std::memcpy(gam_out, gam, sizeof gam);
    return DPENV_OK;
}

// ---- the baseline DP controller's allocation and numbers (dpenv.h) ------------------------------------------------------------------
extern "C" int dpenv_dp_allocation_matrix(const float lx[3], const float ly[3], const float weight[5], float G_out[5][3])
{
    if (!lx || !ly || !weight || !G_out) return fail(nullptr, DPENV_EINVAL, "dpenv_dp_allocation_matrix: NULL argument");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(lx[k]) || !std::isfinite(ly[k])) return fail(nullptr, DPENV_EINVAL, "dpenv_dp_allocation_matrix: lever arms must be finite");
    for (int k = 0; k < 5; ++k)
        if (!std::isfinite(weight[k]) || !(weight[k] > 0.0f)) return fail(nullptr, DPENV_EINVAL, "dpenv_dp_allocation_matrix: weight[%d] must be finite and > 0", k);
    // deploy.allocation_matrix is the same recipe in the same order: V = W^-1 T', M = T V, G = V adj(M) / det(M)
    const double T[3][5] = {{0.0, 1.0, 0.0, 1.0, 0.0},
                            {1.0, 0.0, 1.0, 0.0, 1.0},
                            {(double)lx[0], -(double)ly[1], (double)lx[1], -(double)ly[2], (double)lx[2]}};
    double V[5][3], M[3][3];
    for (int m = 0; m < 5; ++m) for (int j = 0; j < 3; ++j) V[m][j] = T[j][m] / (double)weight[m];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) {
        double acc = 0.0;
        for (int m = 0; m < 5; ++m) acc += T[r][m] * V[m][c];
        M[r][c] = acc;
    }
    double adj[3][3];                                            // adj[r][c] = cofactor of M[c][r]
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) {
        const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
        adj[r][c] = M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1];
    }
    const double det = (M[0][0] * adj[0][0] + M[0][1] * adj[1][0]) + M[0][2] * adj[2][0];
    if (!std::isfinite(det) || det == 0.0) return fail(nullptr, DPENV_EINVAL, "dpenv_dp_allocation_matrix: T W^-1 T' is singular");
    for (int m = 0; m < 5; ++m) for (int c = 0; c < 3; ++c) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += V[m][j] * adj[j][c];
        G_out[m][c] = (float)(acc / det);
    }
    return DPENV_OK;
}

const char* host::control_check(const dpenv_dp_controller* c, ControlArgs& g)
{
    if (c->struct_size != sizeof(dpenv_dp_controller)) return "dpenv_dp_controller ABI mismatch";
    for (int j = 0; j < 3; ++j) {
        if (!std::isfinite(c->kp[j]) || !std::isfinite(c->kd[j]) || !std::isfinite(c->ki[j])) return "DP controller: kp, kd and ki must be finite";
        if (std::isnan(c->z_bound[j]) || c->z_bound[j] < 0.0f) return "DP controller: z_bound must be >= 0";
        if (std::isnan(c->tau_max[j]) || c->tau_max[j] < 0.0f) return "DP controller: tau_max must be >= 0";
        if (!std::isfinite(c->kf[j]) || !(c->kf[j] > 0.0f)) return "DP controller: kf must be finite and > 0";
    }
    if (!std::isfinite(c->kr_bow) || !(c->kr_bow > 0.0f)) return "DP controller: kr_bow must be finite and > 0";
    if (std::isnan(c->f_eps) || c->f_eps < 0.0f) return "DP controller: f_eps must be >= 0";
    for (int m = 0; m < 5; ++m) for (int j = 0; j < 3; ++j) if (!std::isfinite(c->G[m][j])) return "DP controller: G must be finite";
    for (int j = 0; j < 3; ++j) {
        g.kp[j] = c->kp[j]; g.kd[j] = c->kd[j]; g.ki[j] = c->ki[j]; g.zb[j] = c->z_bound[j]; g.tmax[j] = c->tau_max[j]; g.kf[j] = c->kf[j];
    }
    std::memcpy(g.G, c->G, sizeof g.G);
    g.kr_bow = c->kr_bow;
    g.f_eps = c->f_eps;
    return nullptr;
}

extern "C" int dpenv_thrust_alloc(const dpenv_dp_controller* c, const float* tau, float* action_out, int32_t n, dpenv_stream s)
{
    if (!c || !tau || !action_out || n <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc: bad argument");
    ControlArgs g = {};
    if (const char* why = control_check(c, g)) return fail(nullptr, DPENV_EINVAL, "%s", why);
    HIP_TRY(nullptr, dev::launch_thrust_alloc(&g, tau, action_out, n, (hipStream_t)s));
    return DPENV_OK;
}

// ---- the rate-limited QP thrust allocation (dpenv.h; the kernel is dpenv_control.hip's) ------------------------------------------------
extern "C" int dpenv_qp_allocator_defaults(dpenv_qp_allocator* q)
{
    if (!q) return fail(nullptr, DPENV_EINVAL, "dpenv_qp_allocator_defaults: q is NULL");
    std::memset(q, 0, sizeof *q);
    q->struct_size = (uint32_t)sizeof *q;
    q->iterations = 16;
    float v[DPENV_NPARAM];
    dpenv_default_vessel(v);
    const float f_max[3] = {9.0f, 20.5f, 20.5f};                 // qp_allocator.py:52, env order
    const float rate[3] = {10.0f, 25.0f, 25.0f};                 // :57: 2, 5, 5 N per 0.2 s step
    for (int k = 0; k < 3; ++k) {
        q->w_slack[k] = 1.0f;                                    // :116-150
        q->f_max[k] = f_max[k];
        q->force_rate[k] = rate[k];
        q->lx[k] = v[DPENV_P_LX_BOW + k]; q->ly[k] = v[DPENV_P_LY_BOW + k];
        q->kf[k] = v[DPENV_P_KF_BOW + k]; q->kr[k] = v[DPENV_P_KR_BOW + k];
    }
    q->w_power = 1.0f;
    q->w_dalpha = q->w_dforce = 0.25f;
    q->azimuth_rate[0] = q->azimuth_rate[1] = (float)(5.0 * 3.14159265358979323846 / 12.0);   // :58: pi / 12 per 0.2 s step
    return DPENV_OK;
}

// validates q and dt and forms the kernel's numbers; the reason for a refusal, or NULL
const char* host::qp_check(const dpenv_qp_allocator* q, float dt, QpArgs& g)
{
    if (q->struct_size != sizeof(dpenv_qp_allocator)) return "dpenv_qp_allocator ABI mismatch";
    if (q->iterations < 1 || q->iterations > QP_MAX_ITERS) return "QP allocator: iterations must be in 1..32";
    if (!std::isfinite(dt) || !(dt > 0.0f)) return "QP allocator: dt must be finite and > 0";
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(q->w_slack[k]) || q->w_slack[k] < 0.0f) return "QP allocator: w_slack must be finite and >= 0";
        if (!std::isfinite(q->f_max[k]) || q->f_max[k] < 0.0f) return "QP allocator: f_max must be finite and >= 0";
        if (!std::isfinite(q->force_rate[k]) || q->force_rate[k] < 0.0f) return "QP allocator: force_rate must be finite and >= 0";
        if (!std::isfinite(q->lx[k]) || !std::isfinite(q->ly[k])) return "QP allocator: lever arms must be finite";
        if (!std::isfinite(q->kf[k]) || !(q->kf[k] > 0.0f)) return "QP allocator: kf must be finite and > 0";
        if (!std::isfinite(q->kr[k]) || !(q->kr[k] > 0.0f)) return "QP allocator: kr must be finite and > 0";
    }
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(q->azimuth_rate[k]) || q->azimuth_rate[k] < 0.0f) return "QP allocator: azimuth_rate must be finite and >= 0";
    if (!std::isfinite(q->w_power) || q->w_power < 0.0f) return "QP allocator: w_power must be finite and >= 0";
    if (!std::isfinite(q->w_dalpha) || !(q->w_dalpha > 0.0f)) return "QP allocator: w_dalpha must be finite and > 0";
    if (!std::isfinite(q->w_dforce) || !(q->w_dforce > 0.0f)) return "QP allocator: w_dforce must be finite and > 0";
    for (int k = 0; k < 3; ++k) {
        g.ws[k] = q->w_slack[k]; g.fmax[k] = q->f_max[k]; g.dF[k] = q->force_rate[k] * dt;
        g.lx[k] = q->lx[k]; g.ly[k] = q->ly[k]; g.kf[k] = q->kf[k]; g.kr[k] = q->kr[k];
        if (!std::isfinite(g.dF[k])) return "QP allocator: force_rate * dt overflows";
    }
    for (int k = 0; k < 2; ++k) {
        g.da[k] = q->azimuth_rate[k] * dt;
        if (!std::isfinite(g.da[k])) return "QP allocator: azimuth_rate * dt overflows";
    }
    g.wp = q->w_power; g.wda = q->w_dalpha; g.wdf = q->w_dforce;
    g.iters = q->iterations;
    return nullptr;
}

extern "C" int dpenv_thrust_alloc_qp(const dpenv_qp_allocator* q, float dt, const float* tau, const float* state_in, float* state_out,
                                     float* action_out, float* cost_out, int32_t n, dpenv_stream s)
{
    if (!q || !tau || !action_out || n <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_qp: bad argument");
    QpArgs g = {};
    if (const char* why = qp_check(q, dt, g)) return fail(nullptr, DPENV_EINVAL, "%s", why);
    const QpAllocIO io = {tau, state_in, state_out, action_out, cost_out, n};
    HIP_TRY(nullptr, dev::launch_qp_alloc(&g, &io, (hipStream_t)s));
    return DPENV_OK;
}

// ... with row i of the public table on env i: the lane checks its own row (no packing launch, one kernel node)
extern "C" int dpenv_thrust_alloc_qp_table(const float* table, int32_t iterations, float dt, const float* tau, const float* state_in,
                                           float* state_out, float* action_out, float* cost_out, uint8_t* refused_out, int32_t n,
                                           dpenv_stream s)
{
    if (!table || !tau || !action_out || n <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_qp_table: bad argument");
    if (iterations < 1 || iterations > QP_MAX_ITERS) return fail(nullptr, DPENV_EINVAL, "QP allocator: iterations must be in 1..32");
    if (!std::isfinite(dt) || !(dt > 0.0f)) return fail(nullptr, DPENV_EINVAL, "QP allocator: dt must be finite and > 0");
    const QpAllocIO io = {tau, state_in, state_out, action_out, cost_out, n};
    HIP_TRY(nullptr, dev::launch_qp_alloc_tab(table, iterations, dt, &io, refused_out, (hipStream_t)s));
    return DPENV_OK;
}

// ---- the neural thrust allocation (dpenv.h; the kernels are dpenv_control_nn.hip's) ------------------------------------------------------
extern "C" int dpenv_nn_allocator_defaults(dpenv_nn_allocator* a)
{
    if (!a) return fail(nullptr, DPENV_EINVAL, "dpenv_nn_allocator_defaults: a is NULL");
    std::memset(a, 0, sizeof *a);
    a->struct_size = (uint32_t)sizeof *a;
    const float l[6] = {-1.12f, -0.15f, -1.12f, 0.15f, 1.08f, 0.0f};     // neural_allocator.py:74-79: lx, ly of port, star, bow
    for (int k = 0; k < 6; ++k) a->in_const[k] = l[k];
    a->tau_scale[0] = (float)(1.0 / 54.0);                               // :60
    a->tau_scale[1] = (float)(1.0 / 69.2);
    a->tau_scale[2] = (float)(1.0 / 76.9);
    a->angle_scale = (float)3.14159265358979323846;                      // :50,61
    a->azimuth_mode = 0;
    a->azimuth[0] = (float)(-3.0 * 3.14159265358979323846 / 4.0);        // :225
    a->azimuth[1] = (float)(3.0 * 3.14159265358979323846 / 4.0);
    a->device_pointers = 1;
    return DPENV_OK;
}

// validates a and forms the kernel's numbers; the reason for a refusal, or NULL
const char* host::nn_check(const dpenv_nn_allocator* a, NnArgs& g)
{
    if (a->struct_size != sizeof(dpenv_nn_allocator)) return "dpenv_nn_allocator ABI mismatch (struct_size)";
    const dpenv_mlp* m = a->net;
    if (!m) return "NN allocator: net is NULL";
    if (m->n_layers < 2 || m->n_layers > NN_MAX_LAYERS) return "NN allocator: net n_layers must be in 2..5";
    const int L = m->n_layers;
    if (m->sizes[0] != 3 && m->sizes[0] != 9) return "NN allocator: net sizes[0] must be 3 or 9";
    if (m->sizes[L] != 6) return "NN allocator: net sizes[n_layers] must be 6";
    for (int l = 1; l < L; ++l)
        if (m->sizes[l] < 1 || m->sizes[l] > NN_MAX_H || m->sizes[l] != m->sizes[1]) return "NN allocator: net hidden sizes must be equal and in 1..96";
    for (int l = 0; l < L; ++l)
        if (!m->W[l] || !m->b[l]) return "NN allocator: net W and b must not be NULL";
    if (!std::isfinite(a->leak) || a->leak < 0.0f || a->leak > 1.0f) return "NN allocator: leak must be in [0, 1]";
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(a->in_const[k])) return "NN allocator: in_const must be finite";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(a->tau_scale[k])) return "NN allocator: tau_scale must be finite";
    if (!std::isfinite(a->angle_scale)) return "NN allocator: angle_scale must be finite";
    if (a->azimuth_mode != 0 && a->azimuth_mode != 1) return "NN allocator: azimuth_mode must be 0 or 1";
    if (!std::isfinite(a->azimuth[0]) || !std::isfinite(a->azimuth[1])) return "NN allocator: azimuth must be finite";
    g = NnArgs{};
    for (int l = 0; l < L; ++l) { g.W[l] = m->W[l]; g.b[l] = m->b[l]; }
    g.n_layers = L; g.in_dim = m->sizes[0]; g.H = m->sizes[1];
    g.leak = a->leak;
    for (int k = 0; k < 6; ++k) g.in_const[k] = a->in_const[k];
    for (int k = 0; k < 3; ++k) g.tau_scale[k] = a->tau_scale[k];
    g.angle_scale = a->angle_scale;
    g.azimuth_mode = a->azimuth_mode;
    g.azimuth[0] = a->azimuth[0]; g.azimuth[1] = a->azimuth[1];
    return nullptr;
}

// ... for the calls that read the weights where they are (dpenv_thrust_alloc_nn, dpenv_controller_label_nn with a network of its own)
const char* host::nn_check_in_place(const dpenv_nn_allocator* a, NnArgs& g)
{
    if (const char* why = nn_check(a, g)) return why;
    if (a->device_pointers != 1) return "NN allocator: device_pointers must be 1 (the weights are read in place)";
    return nullptr;
}

extern "C" int dpenv_thrust_alloc_nn(const dpenv_nn_allocator* a, const float* tau, float* action_out, float* raw_out, int32_t n, dpenv_stream s)
{
    if (!a) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_nn: a is NULL");
    if (!tau || !action_out) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_nn: tau and action_out must not be NULL");
    if (n <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_nn: n must be > 0");
    NnArgs g;
    if (const char* why = nn_check_in_place(a, g)) return fail(nullptr, DPENV_EINVAL, "%s", why);
    HIP_TRY(nullptr, dev::launch_nn_alloc(&g, tau, action_out, raw_out, n, (hipStream_t)s));
    return DPENV_OK;
}

const char* host::nn_pop_check(int32_t K, int32_t envs_per_net)
{
    if (K < 1) return "K must be >= 1";
    if (envs_per_net < 64 || envs_per_net % 64 != 0) return "envs_per_net must be a multiple of 64, >= 64 (a wave flies one network)";
    if ((int64_t)K * (envs_per_net / 64) >= ((int64_t)1 << 31)) return "K * (envs_per_net / 64) must be below 2^31";
    return nullptr;
}

extern "C" int dpenv_thrust_alloc_nn_population(const dpenv_nn_allocator* a, int32_t K, int32_t envs_per_net, const float* tau,
                                                float* action_out, float* raw_out, int32_t n, dpenv_stream s)
{
    if (!a) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_nn_population: a is NULL");
    if (!tau || !action_out) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_nn_population: tau and action_out must not be NULL");
    if (n <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_nn_population: n must be > 0");
    NnPop p = {};
    if (const char* why = nn_check_in_place(a, p.a)) return fail(nullptr, DPENV_EINVAL, "%s", why);
    if (const char* why = nn_pop_check(K, envs_per_net)) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_alloc_nn_population: %s", why);
    p.K = K; p.waves_per_net = envs_per_net / 64; p.wave_base = 0;
    HIP_TRY(nullptr, dev::launch_nn_alloc_pop(&p, tau, action_out, raw_out, n, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_thrust_map(const float* params, const float* n_pct, const float* alpha, float* tau_out, int32_t n,
                                dpenv_stream s)
{
    if (!n_pct || !alpha || !tau_out || n <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_thrust_map: bad argument");
    float defp[DPENV_NPARAM];
    if (!params) { dpenv_default_vessel(defp); params = defp; }
    VesselDev vd;
    std::string why;
    if (derive_vessel(params, &vd, &why, true) != DPENV_OK) return fail(nullptr, DPENV_EINVAL, "%s", why.c_str());
    HIP_TRY(nullptr, dev::launch_thrust_map(&vd, n_pct, alpha, tau_out, n, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int64_t dpenv_gae_workspace_bytes(int32_t n) { return n > 0 ? dev::gae_workspace_bytes(n) : 0; }

extern "C" int dpenv_gae_stats(const float* rew, const float* val, const uint8_t* end, const float* boot, const float* last_val,
                               int32_t T, int32_t n, float gamma, float lam, float* adv_out, float* ret_out, void* workspace,
                               double* stats_out, dpenv_stream s)
{
    if (!rew || !val || !adv_out || !ret_out || T <= 0 || n <= 0)
        return fail(nullptr, DPENV_EINVAL, "dpenv_gae: bad argument");
    if (stats_out && !workspace) return fail(nullptr, DPENV_EINVAL, "dpenv_gae_stats: statistics need the workspace (dpenv_gae_workspace_bytes)");
    HIP_TRY(nullptr, dev::launch_gae(rew, val, end, boot, last_val, T, n, gamma, lam, adv_out, ret_out, (double*)workspace,
                                          stats_out, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_gae(const float* rew, const float* val, const uint8_t* end, const float* boot, const float* last_val,
                         int32_t T, int32_t n, float gamma, float lam, float* adv_out, float* ret_out, dpenv_stream s)
{
    return dpenv_gae_stats(rew, val, end, boot, last_val, T, n, gamma, lam, adv_out, ret_out, nullptr, nullptr, s);
}

// ---- streaming score card (dpenv.h: dpenv_score_*): handle-free; every argument is validated here, before any device call ----
extern "C" int64_t dpenv_score_state_bytes(int32_t n) { return n > 0 ? dev::score_state_bytes(n) : 0; }

extern "C" int64_t dpenv_score_summary_workspace_bytes(int32_t n) { return n > 0 ? dev::score_summary_workspace_bytes(n) : 0; }

extern "C" int dpenv_score_default_io(dpenv_score_io* io)
{
    if (!io) return fail(nullptr, DPENV_EINVAL, "dpenv_score_default_io: io is NULL");
    std::memset(io, 0, sizeof *io);
    io->struct_size = (uint32_t)sizeof *io;
    io->obs_dtype = DPENV_F32;
    io->obs_stride = 9;
    io->act_stride = 7;
    io->dt = 0.2f;
    const double kq0[3] = {0.02, 0.036, 0.036}, diam[3] = {0.06, 0.15, 0.15};
    const float norm[3] = {5.0f, 5.0f, 25.0f}, rps[3] = {33.0f, 11.0f, 11.0f};
    for (int j = 0; j < 3; ++j) {
        io->norm[j] = norm[j];
        io->rps_max[j] = rps[j];
        const double d = diam[j];
        io->power_coeff[j] = (float)(kq0[j] * 2 * 3.141592653589793 * 1025.0 * (d * d * d * d * d));
    }
    return DPENV_OK;
}

// what dpenv_score_accumulate and dpenv_score_accumulate_wear both refuse (who: the entry point named in the message), then the kernel's arguments
static int score_check(const char* who, void* state, const dpenv_score_io* io, ScoreArgs* a)
{
    if (!io) return fail(nullptr, DPENV_EINVAL, "%s: io is NULL", who);
    if (io->struct_size != sizeof(dpenv_score_io))
        return fail(nullptr, DPENV_EINVAL, "%s: struct_size %u != %zu", who, io->struct_size, sizeof(dpenv_score_io));
    if (io->T < 1) return fail(nullptr, DPENV_EINVAL, "%s: T = %d, must be >= 1", who, io->T);
    if (io->n < 1) return fail(nullptr, DPENV_EINVAL, "%s: n = %d, must be >= 1", who, io->n);
    if (!state) return fail(nullptr, DPENV_EINVAL, "%s: state is NULL", who);
    if (reinterpret_cast<uintptr_t>(state) & 15u) return fail(nullptr, DPENV_EINVAL, "%s: state must be 16-byte aligned", who);
    if (io->obs_dtype != DPENV_F32 && io->obs_dtype != DPENV_BF16)
        return fail(nullptr, DPENV_EINVAL, "%s: obs_dtype %d is neither DPENV_F32 nor DPENV_BF16", who, io->obs_dtype);
    if (io->obs && io->obs_stride < 3) return fail(nullptr, DPENV_EINVAL, "%s: obs_stride = %d, must be >= 3", who, io->obs_stride);
    if (io->act && io->act_stride < 3) return fail(nullptr, DPENV_EINVAL, "%s: act_stride = %d, must be >= 3", who, io->act_stride);
    if (io->integ && !io->obs) return fail(nullptr, DPENV_EINVAL, "%s: integ needs obs", who);
    if (!std::isfinite(io->dt) || !(io->dt > 0.0f)) return fail(nullptr, DPENV_EINVAL, "%s: dt must be finite and > 0", who);
    for (int j = 0; j < 3; ++j) {
        if (!std::isfinite(io->norm[j]) || !(io->norm[j] > 0.0f))
            return fail(nullptr, DPENV_EINVAL, "%s: norm[%d] must be finite and > 0", who, j);
        if (!std::isfinite(io->power_coeff[j])) return fail(nullptr, DPENV_EINVAL, "%s: power_coeff[%d] is not finite", who, j);
        if (!std::isfinite(io->rps_max[j])) return fail(nullptr, DPENV_EINVAL, "%s: rps_max[%d] is not finite", who, j);
    }
    a->state = (uint4*)state;
    a->obs = io->obs; a->act = io->act; a->rew = io->rew; a->done = io->done; a->integ = io->integ;
    a->T = io->T; a->n = io->n; a->obs_stride = io->obs_stride; a->act_stride = io->act_stride; a->cut_at_end = io->cut_at_end ? 1 : 0;
    a->dt = io->dt;
    for (int j = 0; j < 3; ++j) { a->norm[j] = io->norm[j]; a->coeff[j] = io->power_coeff[j]; a->rps[j] = io->rps_max[j]; }
    return DPENV_OK;
}

extern "C" int dpenv_score_accumulate(void* state, const dpenv_score_io* io, dpenv_stream s)
{
    ScoreArgs a;
    if (int rc = score_check("dpenv_score_accumulate", state, io, &a)) return rc;
    HIP_TRY(nullptr, dev::launch_score(&a, io->obs_dtype == DPENV_BF16, (hipStream_t)s));
    return DPENV_OK;
}

// ---- the wear axis (dpenv.h: dpenv_score_accumulate_wear, dpenv_score_wear_*): IADC beside the score state, one pass over the rows ----
extern "C" int64_t dpenv_score_wear_state_bytes(int32_t n) { return n > 0 ? dev::score_wear_state_bytes(n) : 0; }

extern "C" int64_t dpenv_score_wear_summary_workspace_bytes(int32_t n) { return n > 0 ? dev::score_wear_summary_workspace_bytes(n) : 0; }

extern "C" int dpenv_score_accumulate_wear(void* state, void* wear, const dpenv_score_io* io, const dpenv_score_wear_io* wio, dpenv_stream s)
{
    static const char* who = "dpenv_score_accumulate_wear";
    ScoreArgs a;
    if (int rc = score_check(who, state, io, &a)) return rc;
    if (!wear) return fail(nullptr, DPENV_EINVAL, "%s: wear is NULL", who);
    if (reinterpret_cast<uintptr_t>(wear) & 15u) return fail(nullptr, DPENV_EINVAL, "%s: wear must be 16-byte aligned", who);
    if (!wio) return fail(nullptr, DPENV_EINVAL, "%s: wio is NULL", who);
    if (wio->struct_size != sizeof(dpenv_score_wear_io))
        return fail(nullptr, DPENV_EINVAL, "%s: wio struct_size %u != %zu", who, wio->struct_size, sizeof(dpenv_score_wear_io));
    dpenv_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.variant = wio->variant; cfg.cont_ang = wio->cont_ang;
    const int mode = mode_of(&cfg);
    if (mode < 0) return fail(nullptr, DPENV_EINVAL, "%s: variant %d is none of DPENV_FULL .. DPENV_FINAL", who, wio->variant);
    if (wio->cont_ang && wio->variant != DPENV_FINAL)
        return fail(nullptr, DPENV_EINVAL, "%s: cont_ang is only defined for the final variant", who);
    if (!io->act) return fail(nullptr, DPENV_EINVAL, "%s: act is NULL (the wear axis is taken on the action rows)", who);
    const int ad = dpenv_act_dim(&cfg);
    if (io->act_stride < ad)
        return fail(nullptr, DPENV_EINVAL, "%s: act_stride = %d, must be >= %d (the variant's dpenv_act_dim)", who, io->act_stride, ad);
    HIP_TRY(nullptr, dev::launch_score_wear(&a, wear, io->obs_dtype == DPENV_BF16, mode, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_score_wear_read(const void* wear, int32_t n, double* out, dpenv_stream s)
{
    if (n < 1) return fail(nullptr, DPENV_EINVAL, "dpenv_score_wear_read: n = %d, must be >= 1", n);
    if (!wear || (reinterpret_cast<uintptr_t>(wear) & 15u)) return fail(nullptr, DPENV_EINVAL, "dpenv_score_wear_read: wear is NULL or not 16-byte aligned");
    if (!out) return fail(nullptr, DPENV_EINVAL, "dpenv_score_wear_read: out is NULL");
    HIP_TRY(nullptr, dev::launch_score_wear_read(wear, n, out, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_score_wear_summary(const void* wear, int32_t n, double* out, void* workspace, dpenv_stream s)
{
    if (n < 1) return fail(nullptr, DPENV_EINVAL, "dpenv_score_wear_summary: n = %d, must be >= 1", n);
    if (!wear || (reinterpret_cast<uintptr_t>(wear) & 15u)) return fail(nullptr, DPENV_EINVAL, "dpenv_score_wear_summary: wear is NULL or not 16-byte aligned");
    if (!out) return fail(nullptr, DPENV_EINVAL, "dpenv_score_wear_summary: out is NULL");
    if (!workspace) return fail(nullptr, DPENV_EINVAL, "dpenv_score_wear_summary: workspace is NULL (dpenv_score_wear_summary_workspace_bytes)");
    HIP_TRY(nullptr, dev::launch_score_wear_summary(wear, n, out, (double*)workspace, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_score_read(const void* state, int32_t n, double* out, dpenv_stream s)
{
    if (n < 1) return fail(nullptr, DPENV_EINVAL, "dpenv_score_read: n = %d, must be >= 1", n);
    if (!state || (reinterpret_cast<uintptr_t>(state) & 15u)) return fail(nullptr, DPENV_EINVAL, "dpenv_score_read: state is NULL or not 16-byte aligned");
    if (!out) return fail(nullptr, DPENV_EINVAL, "dpenv_score_read: out is NULL");
    HIP_TRY(nullptr, dev::launch_score_read(state, n, out, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_score_summary(const void* state, int32_t n, double* out, void* workspace, dpenv_stream s)
{
    if (n < 1) return fail(nullptr, DPENV_EINVAL, "dpenv_score_summary: n = %d, must be >= 1", n);
    if (!state || (reinterpret_cast<uintptr_t>(state) & 15u)) return fail(nullptr, DPENV_EINVAL, "dpenv_score_summary: state is NULL or not 16-byte aligned");
    if (!out) return fail(nullptr, DPENV_EINVAL, "dpenv_score_summary: out is NULL");
    if (!workspace) return fail(nullptr, DPENV_EINVAL, "dpenv_score_summary: workspace is NULL (dpenv_score_summary_workspace_bytes)");
    HIP_TRY(nullptr, dev::launch_score_summary(state, n, out, (double*)workspace, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_adv_sum(const float* adv, int64_t count, float* sum_out, dpenv_stream s)
{
    if (!adv || !sum_out || count <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_adv_sum: bad argument");
    HIP_TRY(nullptr, dev::launch_sum(adv, count, nullptr, sum_out, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_adv_sumsq(const float* adv, int64_t count, const float* mean, float* sumsq_out, dpenv_stream s)
{
    if (!adv || !mean || !sumsq_out || count <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_adv_sumsq: bad argument");
    HIP_TRY(nullptr, dev::launch_sum(adv, count, mean, sumsq_out, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_adv_apply(float* adv, int64_t count, const float* mean, const float* std, dpenv_stream s)
{
    if (!adv || !mean || !std || count <= 0) return fail(nullptr, DPENV_EINVAL, "dpenv_adv_apply: bad argument");
    HIP_TRY(nullptr, dev::launch_adv_apply(adv, count, mean, std, nullptr, 0.0, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_adv_apply_stats(float* adv, int64_t count, const double* stats, double total_count, dpenv_stream s)
{
    if (!adv || !stats || count <= 0 || !(total_count >= 1.0)) return fail(nullptr, DPENV_EINVAL, "dpenv_adv_apply_stats: bad argument");
    HIP_TRY(nullptr, dev::launch_adv_apply(adv, count, nullptr, nullptr, stats, total_count, (hipStream_t)s));
    return DPENV_OK;
}

// ---- the PPO update (dpenv.h: dpenv_ppo_actor_grad, dpenv_value_grad, dpenv_adam_step): every argument is validated here, before any device call ----
static const char* train_shape_check(const dpenv_train_shape* sh, TrainLayout* L)
{
    if (!sh) return "shape is NULL";
    if (sh->struct_size != sizeof(dpenv_train_shape)) return "dpenv_train_shape ABI mismatch";
    if (sh->row_dtype != DPENV_F32) return "rows must be DPENV_F32 (bf16 rows are not implemented)";
    if (sh->activation != DPENV_ACT_LEAKY_RELU) return "activation must be DPENV_ACT_LEAKY_RELU (tanh is not implemented)";
    if (!(sh->leak >= 0.0f && sh->leak <= 1.0f)) return "leak must be in [0, 1]";
    if (sh->n_layers != 4) return "n_layers must be 4 (in -> 80 -> 80 -> 80 -> out)";
    if (sh->sizes[1] != TR_H || sh->sizes[2] != TR_H || sh->sizes[3] != TR_H) return "the three hidden layers must be 80 wide";
    if (sh->sizes[0] < 1 || sh->sizes[0] > TR_PAD) return "the input width must be in 1 .. 16";
    if (sh->log_std != 0 && sh->log_std != 1) return "log_std must be 0 (critic) or 1 (actor)";
    if (sh->log_std ? (sh->sizes[4] < 1 || sh->sizes[4] > 7) : sh->sizes[4] != 1) return "the output width must be 1 .. 7 for an actor and 1 for a critic";
    *L = train_layout(sh->sizes[0], sh->sizes[4], sh->log_std);
    return nullptr;
}

static int64_t train_ws_bytes(const TrainLayout& L, int count)
{
    return (int64_t)train_grid(count) * (L.P + (L.actor ? TR_NSTAT_ACTOR : TR_NSTAT_CRITIC)) * (int64_t)sizeof(float);
}

extern "C" int64_t dpenv_train_param_count(const dpenv_train_shape* shape)
{
    TrainLayout L;
    if (const char* why = train_shape_check(shape, &L)) return fail(nullptr, DPENV_EINVAL, "dpenv_train_param_count: %s", why);
    return L.P;
}

extern "C" int dpenv_train_workspace_bytes(const dpenv_train_shape* shape, int32_t max_count, int64_t* bytes_out)
{
    TrainLayout L;
    if (const char* why = train_shape_check(shape, &L)) return fail(nullptr, DPENV_EINVAL, "dpenv_train_workspace_bytes: %s", why);
    if (!bytes_out) return fail(nullptr, DPENV_EINVAL, "dpenv_train_workspace_bytes: bytes_out is NULL");
    if (max_count < 1 || max_count > TR_MAX_COUNT)
        return fail(nullptr, DPENV_EINVAL, "dpenv_train_workspace_bytes: max_count = %d, must be in 1 .. %d", max_count, TR_MAX_COUNT);
    *bytes_out = train_ws_bytes(L, max_count);
    return DPENV_OK;
}

// what every gradient entry point asks of its row selection and its workspace: the one statement of the limits
static int train_rows_check(const char* who, const TrainLayout& L, const int32_t* idx, int32_t count, int32_t n_rows, const void* workspace,
                            int64_t workspace_bytes)
{
    if (count <= 0) return fail(nullptr, DPENV_EINVAL, "%s: count = %d, must be >= 1", who, count);
    if (count > TR_MAX_COUNT) return fail(nullptr, DPENV_EINVAL, "%s: count = %d, at most %d rows per call", who, count, TR_MAX_COUNT);
    if (n_rows <= 0) return fail(nullptr, DPENV_EINVAL, "%s: n_rows = %d, must be >= 1", who, n_rows);
    if (!idx && n_rows < count) return fail(nullptr, DPENV_EINVAL, "%s: without idx the rows are 0 .. count-1: n_rows = %d < count = %d", who, n_rows, count);
    if (!workspace) return fail(nullptr, DPENV_EINVAL, "%s: workspace is NULL (dpenv_train_workspace_bytes)", who);
    if (reinterpret_cast<uintptr_t>(workspace) & 3u) return fail(nullptr, DPENV_EINVAL, "%s: workspace must be 4-byte aligned", who);
    if (workspace_bytes < train_ws_bytes(L, count))
        return fail(nullptr, DPENV_EINVAL, "%s: workspace of %lld bytes, count = %d needs %lld (dpenv_train_workspace_bytes)", who,
                    (long long)workspace_bytes, count, (long long)train_ws_bytes(L, count));
    return DPENV_OK;
}

static int train_grad(const char* who, const dpenv_train_shape* shape, int actor, const float* theta, const float* obs, const float* act,
                      const float* adv, const float* logp_old, const int32_t* idx, int32_t count, int32_t n_rows, float clip,
                      const int32_t* stop_flag, float* grad_out, void* workspace, int64_t workspace_bytes, dpenv_stream s)
{
    GradArgs a = {};
    if (const char* why = train_shape_check(shape, &a.L)) return fail(nullptr, DPENV_EINVAL, "%s: %s", who, why);
    if (a.L.actor != actor) return fail(nullptr, DPENV_EINVAL, "%s: the shape's log_std = %d is the other network's", who, a.L.actor);
    if (int rc = train_rows_check(who, a.L, idx, count, n_rows, workspace, workspace_bytes)) return rc;
    if (!theta || !obs || !adv || !grad_out) return fail(nullptr, DPENV_EINVAL, "%s: NULL argument", who);
    if (actor && (!act || !logp_old)) return fail(nullptr, DPENV_EINVAL, "%s: NULL argument", who);
    if (actor && !(std::isfinite(clip) && clip >= 0.0f)) return fail(nullptr, DPENV_EINVAL, "%s: clip must be finite and >= 0", who);
    a.theta = theta; a.obs = obs; a.act = act; a.adv = adv; a.logp_old = logp_old; a.idx = idx; a.stop_flag = stop_flag;
    a.partial = (float*)workspace; a.grad_out = grad_out; a.count = count; a.leak = shape->leak; a.clip = clip;
    HIP_TRY(nullptr, dev::launch_mlp_grad(&a, actor ? TR_STAGE_PPO : TR_STAGE_VALUE, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_ppo_actor_grad(const dpenv_train_shape* shape, const float* theta, const float* obs, const float* act, const float* adv,
                                    const float* logp_old, const int32_t* idx, int32_t count, int32_t n_rows, float clip,
                                    const int32_t* stop_flag, float* grad_out, void* workspace, int64_t workspace_bytes, dpenv_stream s)
{
    return train_grad("dpenv_ppo_actor_grad", shape, 1, theta, obs, act, adv, logp_old, idx, count, n_rows, clip, stop_flag, grad_out, workspace,
                      workspace_bytes, s);
}

extern "C" int dpenv_value_grad(const dpenv_train_shape* shape, const float* theta, const float* obs, const float* ret, const int32_t* idx,
                                int32_t count, int32_t n_rows, float* grad_out, void* workspace, int64_t workspace_bytes, dpenv_stream s)
{
    return train_grad("dpenv_value_grad", shape, 0, theta, obs, nullptr, ret, nullptr, idx, count, n_rows, 0.0f, nullptr, grad_out, workspace,
                      workspace_bytes, s);
}

// the weighted imitation loss (dpenv.h, IMITATION LOSS): dpenv_ppo_actor_grad's conventions, every refusal naming its argument
extern "C" int dpenv_imitation_grad(const dpenv_train_shape* shape, const float* theta, const float* obs, const float* act, const float* weight,
                                    const int32_t* idx, int32_t count, int32_t n_rows, int32_t loss, const int32_t* stop_flag, float* grad_out,
                                    void* workspace, int64_t workspace_bytes, dpenv_stream s)
{
    const char* who = "dpenv_imitation_grad";
    GradArgs a = {};
    if (const char* why = train_shape_check(shape, &a.L)) return fail(nullptr, DPENV_EINVAL, "%s: %s", who, why);
    if (!a.L.actor) return fail(nullptr, DPENV_EINVAL, "%s: the shape's log_std = 0 is a critic's; the imitation loss is the actor's", who);
    if (loss != DPENV_IMITATE_NLL && loss != DPENV_IMITATE_MSE)
        return fail(nullptr, DPENV_EINVAL, "%s: loss = %d, must be DPENV_IMITATE_NLL (0) or DPENV_IMITATE_MSE (1)", who, loss);
    if (int rc = train_rows_check(who, a.L, idx, count, n_rows, workspace, workspace_bytes)) return rc;
    if (!theta) return fail(nullptr, DPENV_EINVAL, "%s: theta is NULL", who);
    if (!obs) return fail(nullptr, DPENV_EINVAL, "%s: obs is NULL", who);
    if (!act) return fail(nullptr, DPENV_EINVAL, "%s: act is NULL", who);
    if (!grad_out) return fail(nullptr, DPENV_EINVAL, "%s: grad_out is NULL", who);
    a.theta = theta; a.obs = obs; a.act = act; a.adv = weight; a.logp_old = nullptr; a.idx = idx; a.stop_flag = stop_flag;
    a.partial = (float*)workspace; a.grad_out = grad_out; a.count = count; a.leak = shape->leak; a.clip = 0.0f;
    HIP_TRY(nullptr, dev::launch_mlp_grad(&a, loss == DPENV_IMITATE_NLL ? TR_STAGE_IMIT_NLL : TR_STAGE_IMIT_MSE, (hipStream_t)s));
    return DPENV_OK;
}

// ---- the allocation loss (dpenv.h, ALLOCATION LOSS): dpenv_imitation_grad's conventions with the loss's numbers in a struct of their own ----
extern "C" int dpenv_alloc_loss_defaults(dpenv_alloc_loss* q)
{
    if (!q) return fail(nullptr, DPENV_EINVAL, "dpenv_alloc_loss_defaults: q is NULL");
    dpenv_qp_allocator qp;
    dpenv_nn_allocator nn;
    if (int rc = dpenv_qp_allocator_defaults(&qp)) return rc;
    if (int rc = dpenv_nn_allocator_defaults(&nn)) return rc;
    *q = dpenv_alloc_loss{};
    q->struct_size = sizeof(dpenv_alloc_loss);
    for (int k = 0; k < 3; ++k) {
        q->w_slack[k] = qp.w_slack[k];
        q->lx[k] = qp.lx[k]; q->ly[k] = qp.ly[k]; q->kf[k] = qp.kf[k]; q->kr[k] = qp.kr[k];
    }
    q->w_power = qp.w_power;
    q->w_sat = 100.0f;
    q->angle_scale = nn.angle_scale;
    q->azimuth_mode = nn.azimuth_mode;
    q->azimuth[0] = nn.azimuth[0]; q->azimuth[1] = nn.azimuth[1];
    return DPENV_OK;
}

static const char* alloc_loss_check(const dpenv_alloc_loss* q, AllocLossArgs* out)
{
    if (!q) return "loss is NULL";
    if (q->struct_size != sizeof(dpenv_alloc_loss)) return "dpenv_alloc_loss ABI mismatch (struct_size)";
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(q->w_slack[k]) || q->w_slack[k] < 0.0f) return "w_slack must be finite and >= 0";
        if (!std::isfinite(q->lx[k])) return "lx must be finite";
        if (!std::isfinite(q->ly[k])) return "ly must be finite";
        if (!std::isfinite(q->kf[k]) || q->kf[k] <= 0.0f) return "kf must be finite and > 0";
        if (!std::isfinite(q->kr[k]) || q->kr[k] <= 0.0f) return "kr must be finite and > 0";
    }
    if (!std::isfinite(q->w_power) || q->w_power < 0.0f) return "w_power must be finite and >= 0";
    if (!std::isfinite(q->w_sat) || q->w_sat < 0.0f) return "w_sat must be finite and >= 0";
    if (!std::isfinite(q->angle_scale)) return "angle_scale must be finite";
    if (q->azimuth_mode != 0 && q->azimuth_mode != 1) return "azimuth_mode must be 0 (the network's stern angles) or 1 (fixed at azimuth)";
    if (!std::isfinite(q->azimuth[0]) || !std::isfinite(q->azimuth[1])) return "azimuth must be finite";
    for (int k = 0; k < 3; ++k) {
        out->ws[k] = q->w_slack[k]; out->lx[k] = q->lx[k]; out->ly[k] = q->ly[k]; out->kf[k] = q->kf[k]; out->kr[k] = q->kr[k];
    }
    out->wp = q->w_power; out->wsat = q->w_sat; out->angle_scale = q->angle_scale; out->azimuth_mode = q->azimuth_mode;
    out->azimuth[0] = q->azimuth[0]; out->azimuth[1] = q->azimuth[1];
    return nullptr;
}

extern "C" int dpenv_allocation_grad(const dpenv_train_shape* shape, const dpenv_alloc_loss* loss, const float* theta, const float* x,
                                     const float* tau_rows, const float* weight, const int32_t* idx, int32_t count, int32_t n_rows,
                                     const int32_t* stop_flag, float* grad_out, void* workspace, int64_t workspace_bytes, dpenv_stream s)
{
    const char* who = "dpenv_allocation_grad";
    GradArgs a = {};
    AllocLossArgs q = {};
    if (const char* why = train_shape_check(shape, &a.L)) return fail(nullptr, DPENV_EINVAL, "%s: %s", who, why);
    if (!a.L.actor) return fail(nullptr, DPENV_EINVAL, "%s: the shape's log_std = 0 is a critic's; the allocator is fitted as an actor", who);
    if (a.L.in_dim != 3 && a.L.in_dim != 9)
        return fail(nullptr, DPENV_EINVAL, "%s: sizes[0] = %d, the allocator's input width must be 3 or 9", who, a.L.in_dim);
    if (a.L.out_dim != 6) return fail(nullptr, DPENV_EINVAL, "%s: the output width is %d, the allocator's must be 6", who, a.L.out_dim);
    if (const char* why = alloc_loss_check(loss, &q)) return fail(nullptr, DPENV_EINVAL, "%s: %s", who, why);
    if (int rc = train_rows_check(who, a.L, idx, count, n_rows, workspace, workspace_bytes)) return rc;
    if (!theta) return fail(nullptr, DPENV_EINVAL, "%s: theta is NULL", who);
    if (!x) return fail(nullptr, DPENV_EINVAL, "%s: x is NULL", who);
    if (!tau_rows) return fail(nullptr, DPENV_EINVAL, "%s: tau_rows is NULL", who);
    if (!grad_out) return fail(nullptr, DPENV_EINVAL, "%s: grad_out is NULL", who);
    a.theta = theta; a.obs = x; a.act = tau_rows; a.adv = weight; a.logp_old = nullptr; a.idx = idx; a.stop_flag = stop_flag;
    a.partial = (float*)workspace; a.grad_out = grad_out; a.count = count; a.leak = shape->leak; a.clip = 0.0f;
    HIP_TRY(nullptr, dev::launch_alloc_grad(&a, &q, (hipStream_t)s));
    return DPENV_OK;
}

extern "C" int dpenv_adam_step(float* theta, const float* grad, float* m, float* v, int32_t P, float lr, float beta1, float beta2, float eps,
                               int32_t* step_counter, const float* gate_kl, float kl_limit, int32_t* stop_flag, dpenv_stream s)
{
    if (!theta || !grad || !m || !v || !step_counter) return fail(nullptr, DPENV_EINVAL, "dpenv_adam_step: NULL argument");
    if (P < 1) return fail(nullptr, DPENV_EINVAL, "dpenv_adam_step: P = %d, must be >= 1", P);
    if ((reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15u)
        return fail(nullptr, DPENV_EINVAL, "dpenv_adam_step: theta, grad, m and v must be 16-byte aligned");
    if (!std::isfinite(lr) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps >= 0.0f) || !std::isfinite(eps))
        return fail(nullptr, DPENV_EINVAL, "dpenv_adam_step: lr must be finite, beta1 and beta2 in [0, 1), eps finite and >= 0");
    if (gate_kl && !stop_flag) return fail(nullptr, DPENV_EINVAL, "dpenv_adam_step: the gate (gate_kl) needs stop_flag");
    if (gate_kl && std::isnan(kl_limit)) return fail(nullptr, DPENV_EINVAL, "dpenv_adam_step: kl_limit is NaN");
    AdamArgs a = {};
    a.theta = theta; a.grad = grad; a.m = m; a.v = v; a.P = P; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.step_counter = step_counter; a.gate_kl = gate_kl; a.kl_limit = kl_limit; a.stop_flag = stop_flag;
    HIP_TRY(nullptr, dev::launch_adam_step(&a, (hipStream_t)s));
    return DPENV_OK;
}
