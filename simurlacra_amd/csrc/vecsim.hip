// vecsim.hip -- libvecsim: the C-ABI of include/vecsim.h (host side).  The kernels live in vecsim_kernels.h and are
// compiled per env family (vecsim_family.hip) and for the mixed batches (vecsim_mixed.hip); see build.py.
#include "vecsim_kernels.h"

namespace vs {

__global__ void k_bump_row(int* row) { *row += 1; }

// vs_record_hidden: the caller's hidden state [i * es + j * ds] into row `row` (row < 0: the device-side counter) of the plane
__global__ __launch_bounds__(256) void k_record_hidden(const float* __restrict__ src, long es, long ds, float* __restrict__ plane,
                                                       const int* __restrict__ rec_row, int row, int rows, int width, size_t ld, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int r = row >= 0 ? row : *rec_row;
    if (i >= n || r >= rows) return;
    float* dst = plane + (size_t)r * width * ld + i;
    for (int j = 0; j < width; ++j) dst[(size_t)j * ld] = src[(long)i * es + (long)j * ds];
}

// vs_reset with a mask: the recurrent policy's hidden state of the reset lanes
__global__ __launch_bounds__(256) void k_zero_hidden(float* __restrict__ hid, int rows, size_t ld, const uint8_t* __restrict__ mask, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !mask[i]) return;
    for (int j = 0; j < rows; ++j) hid[(size_t)j * ld + i] = 0.f;
}

// vs_reset with a mask: the discrepancy sums (VS_ROLLOUT_LOSS) of the reset lanes
__global__ __launch_bounds__(256) void k_zero_masked(float* __restrict__ p, const uint8_t* __restrict__ mask, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !mask[i]) return;
    p[i] = 0.f;
}

// ... and `rows` rows of the sensitivity buffers (VS_ROLLOUT_GRAD / _GN / _SENS) of the reset lanes
__global__ __launch_bounds__(256) void k_zero_rows_masked(float* __restrict__ p, int rows, size_t ld, const uint8_t* __restrict__ mask, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !mask[i]) return;
    for (int j = 0; j < rows; ++j) p[(size_t)j * ld + i] = 0.f;
}

// vs_set_policy_playback / vs_set_rollout_target: the caller's table src [n_rec][rw] (rw = rows x width floats per recording)
// into the kernel's recording-minor layout dst [rw][n_rec_ld], 0 in the padding columns n_rec .. n_rec_ld - 1
__global__ __launch_bounds__(256) void k_relay_table(const float* __restrict__ src, int n_rec, int64_t rw, float* __restrict__ dst,
                                                     int n_rec_ld) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= rw * n_rec_ld) return;
    const int64_t m = q / n_rec_ld;
    const int r = (int)(q % n_rec_ld);
    dst[q] = r < n_rec ? src[(int64_t)r * rw + m] : 0.f;
}

// vs_rollout_lengths: per lane, the first recorded step whose done bit is set (words [t / 32][ld], bit t % 32); a lane of a
// population's inert group (wg_set[i / 64] < 0) has no rollout: 0
__global__ __launch_bounds__(256) void k_rollout_lengths(const uint32_t* __restrict__ words, size_t ld, int n, int t_steps,
                                                         long long* __restrict__ lengths, uint8_t* __restrict__ done_last,
                                                         const int* __restrict__ wg_set) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (wg_set && wg_set[i >> 6] < 0) {
        lengths[i] = 0;
        done_last[i] = 0;
        return;
    }
    const int nw = (t_steps + 31) / 32;
    int first = -1;
    for (int w = 0; w < nw && first < 0; ++w) {
        uint32_t bits = words[(size_t)w * ld + i];
        if (w == nw - 1 && (t_steps & 31)) bits &= (1u << (t_steps & 31)) - 1u;  // rows beyond t_steps are not part of it
        if (bits) first = w * 32 + (__ffs((int)bits) - 1);
    }
    lengths[i] = first < 0 ? (long long)t_steps : (long long)first + 1;
    done_last[i] = first >= 0;
}

// vs_set_policy_population: set s of the caller's vectors (n_params floats each) into the packed layout of the policy's
// packer, dst[s * stride + q] = map[q] < 0 ? 0 : src[s * n_params + map[q]] for q < stride (map has `slots` <= stride entries)
__global__ __launch_bounds__(256) void k_pack_population(const float* __restrict__ src, int64_t n_params, int n_sets,
                                                         const int* __restrict__ map, int slots, float* __restrict__ dst, int64_t stride) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= stride) return;
    const int m = q < slots ? map[q] : -1;
    for (int64_t s = blockIdx.y; s < n_sets; s += gridDim.y)
        dst[s * stride + q] = m < 0 ? 0.f : src[s * n_params + m];
}

// ---- vs_returns_scan: y_t = x_t + c y_{t+1} backwards inside every rollout of the packed rows (discounted reward-to-go, GAE).
// A flat segmented scan over ROWS in three launches; a row is the affine map y -> a + m y (step rows: m = c, the final-entry
// row of a rollout: a = y_L, m = 0 -- it cuts the carry), and maps compose as (a1, m1) o (a2, m2) = (a1 + m1 a2, m1 m2).
//   k_returns_scan   a workgroup takes tiles of RT_TILE consecutive rows, whatever rollouts they cut: a wave owns 256 of them as
//                    four 64-row chunks (lane = row: coalesced), scans each chunk backwards with cross-lane moves, chains its
//                    chunks in registers and the four waves through LDS; writes y as if nothing followed the tile
//   k_returns_carry  one thread per rollout: the rows of it that start a tile (at most lengths / RT_TILE) get their true value,
//                    last tile first, then the rollout's first row and out_first
//   k_returns_apply  per tile, the rows of the rollout that runs on into the next tile add c^(distance) times that tile's first row
// Tiles sit at multiples of RT_TILE of the row index in all three, so no launch waits on another workgroup of its own grid.
constexpr int RT_TILE = 1024;

// the rollout of row r: the largest j in [lo, hi] with starts[j] + j <= r (which holds for lo)
__device__ inline int rt_find(const long long* __restrict__ starts, int lo, int hi, long long r) {
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (starts[mid] + mid <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// c^k by squaring, k < 2^BITS: at most k - 1 roundings, as many as the k multiplications of the sequential recurrence
template <int BITS>
__device__ inline float rt_pow(float c, int k) {
    float r = 1.f, b = c;
#pragma unroll
    for (int s = 0; s < BITS; ++s) {
        r = ((k >> s) & 1) ? r * b : r;
        b = b * b;
    }
    return r;
}

// a + m y, where m == 0 CUTS: what lies behind a rollout's final-entry row never reaches it, not even as 0 * NaN or 0 * Inf -- a
// non-finite reward or value stays inside its own rollout, as in the sequential recurrence (m == 0 also for gamma = 0 and when
// c^k underflows: there the rows behind contribute nothing either)
__device__ inline float rt_apply(float a, float m, float y) { return m == 0.f ? a : a + m * y; }

__device__ inline long long rt_end(int n, const long long* __restrict__ lengths, const long long* __restrict__ starts) {
    return starts[n - 1] + (n - 1) + lengths[n - 1] + 1;
}

__global__ __launch_bounds__(256) void k_returns_scan(int n, const long long* __restrict__ lengths, const long long* __restrict__ starts,
                                                      const float* __restrict__ rew, long long rs, const float* __restrict__ values,
                                                      long long vst, const uint8_t* __restrict__ done_last, float gamma, float c, int gae,
                                                      float* __restrict__ out) {
    __shared__ float s_a[4], s_m[4];
    const long long r_first = starts[0], r_end = rt_end(n, lengths, starts);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (long long tile = r_first / RT_TILE + blockIdx.x; tile * RT_TILE < r_end; tile += gridDim.x) {
        const long long S = tile * RT_TILE;
        const long long first = S > r_first ? S : r_first, last = (S + RT_TILE < r_end ? S + RT_TILE : r_end) - 1;
        // the rollouts of the tile: every one owns at least a row, so there are at most last - first + 1 of them
        const int j_lo = rt_find(starts, 0, n - 1, first);
        const long long cap = (long long)j_lo + (last - first);
        const int j_hi = rt_find(starts, j_lo, cap < n - 1 ? (int)cap : n - 1, last);
        float a[4], m[4];
        int jl = j_lo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long r = S + w * 256 + i * 64 + lane;
            a[i] = 0.f;  // rows outside the batch: the identity map
            m[i] = 1.f;
            if (r >= first && r <= last) {
                const long long span = i ? 64 : r - first;  // rows since the row jl was found for
                const int j = rt_find(starts, jl, (long long)jl + span < j_hi ? (int)(jl + span) : j_hi, r);
                jl = j;
                const long long fin = starts[j] + j + lengths[j];
                const float keep = (done_last && done_last[j]) ? 0.f : 1.f;  // the bootstrap value survives a time-out only
                if (r == fin) {
                    a[i] = (values && !gae) ? values[r * vst] * keep : 0.f;
                    m[i] = 0.f;
                } else {
                    float x = rew[r * rs];
                    if (gae) {
                        float vn = values[(r + 1) * vst];
                        if (r + 1 == fin) vn = vn * keep;
                        x = x + gamma * vn - values[r * vst];
                    }
                    a[i] = x;
                    m[i] = c;
                }
            }
        }
        float ac = 0.f, mc = 1.f;  // the map of the wave's rows behind chunk i
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            float ai = a[i], mi = m[i];
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const float a2 = __shfl_down(ai, s), m2 = __shfl_down(mi, s);
                if (lane + s < 64) {
                    ai = rt_apply(ai, mi, a2);
                    mi = mi * m2;
                }
            }
            ai = rt_apply(ai, mi, ac);
            mi = mi * mc;
            a[i] = ai;
            m[i] = mi;
            ac = __shfl(ai, 0);
            mc = __shfl(mi, 0);
        }
        if (lane == 0) {
            s_a[w] = ac;
            s_m[w] = mc;
        }
        __syncthreads();
        float carry = 0.f;  // y of the first row of the next wave, as if nothing followed the tile
        for (int k = 3; k > w; --k) carry = rt_apply(s_a[k], s_m[k], carry);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long r = S + w * 256 + i * 64 + lane;
            if (r >= first && r <= last) out[r] = rt_apply(a[i], m[i], carry);
        }
    }
}

__global__ __launch_bounds__(256) void k_returns_carry(int n, const long long* __restrict__ lengths, const long long* __restrict__ starts,
                                                       float c, float* __restrict__ out, float* __restrict__ out_first) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const long long base = starts[j] + j, fin = base + lengths[j];
    const long long e_first = (base / RT_TILE + 1) * RT_TILE;  // the first tile edge behind the rollout's first row
    float y0 = out[base];
    if (e_first <= fin) {
        const long long e_last = fin / RT_TILE * RT_TILE;  // the rollout ends in the tile that starts here: out[e_last] is final
        float carry = out[e_last];
        if (e_last > e_first) {
            const float ct = rt_pow<11>(c, RT_TILE);
            for (long long e = e_last - RT_TILE; e >= e_first; e -= RT_TILE) {
                carry = out[e] + ct * carry;
                out[e] = carry;
            }
        }
        y0 = y0 + rt_pow<11>(c, (int)(e_first - base)) * carry;
        out[base] = y0;
    }
    if (out_first) out_first[j] = y0;
}

__global__ __launch_bounds__(256) void k_returns_apply(int n, const long long* __restrict__ lengths, const long long* __restrict__ starts,
                                                       float c, float* __restrict__ out) {
    const long long r_first = starts[0], r_end = rt_end(n, lengths, starts);
    for (long long tile = r_first / RT_TILE + blockIdx.x; (tile + 1) * RT_TILE < r_end; tile += gridDim.x) {
        const long long S = tile * RT_TILE, E = S + RT_TILE;
        const int j = rt_find(starts, 0, n - 1, E - 1);  // the rollout of the tile's last row ...
        const long long base = starts[j] + j;
        if (base + lengths[j] < E) continue;  // ... ends with it: nothing to carry in
        const float carry = out[E];           // (k_returns_carry's; no workgroup of this launch writes a row that starts a tile)
        for (long long r = (S > base ? S : base) + 1 + threadIdx.x; r < E; r += 256)
            out[r] = out[r] + rt_pow<10>(c, (int)(E - r)) * carry;
    }
}

__global__ void k_count_err(const uint8_t* err, int n, unsigned long long* out) {
    int i = blockIdx.x * BLOCK + threadIdx.x;
    bool e = i < n && err[i] != 0;
    unsigned long long m = __builtin_amdgcn_ballot_w64(e);
    if (__lane_id() == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}

// HBM reference points next to the roofline: a streaming float4 copy and a pure float4 write stream.
// One-shot grids (a block owns PROBE_V * 256 consecutive float4: 16 KiB), PROBE_V independent 16-B accesses per thread in
// flight, non-temporal (the data is touched once).
constexpr int PROBE_V = 4;
typedef float v4f __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_fill4(v4f* __restrict__ dst, size_t n4, float v) {
    size_t base = (size_t)blockIdx.x * (256 * PROBE_V) + threadIdx.x;
    const v4f x = {v, v + 1.f, v + 2.f, v + 3.f};
#pragma unroll
    for (int k = 0; k < PROBE_V; ++k) {
        size_t i = base + (size_t)k * 256;
        if (i < n4) __builtin_nontemporal_store(x, &dst[i]);
    }
}

__global__ __launch_bounds__(256) void k_copy4(const v4f* __restrict__ src, v4f* __restrict__ dst, size_t n4) {
    size_t base = (size_t)blockIdx.x * (256 * PROBE_V) + threadIdx.x;
    v4f x[PROBE_V];
#pragma unroll
    for (int k = 0; k < PROBE_V; ++k) {
        size_t i = base + (size_t)k * 256;
        if (i < n4) x[k] = __builtin_nontemporal_load(&src[i]);
    }
#pragma unroll
    for (int k = 0; k < PROBE_V; ++k) {
        size_t i = base + (size_t)k * 256;
        if (i < n4) __builtin_nontemporal_store(x[k], &dst[i]);
    }
}

}  // namespace vs

// ====================================================================================================================
// host side
// ====================================================================================================================
// ====================================================================================================================
// host side
// ====================================================================================================================
using namespace vs;

struct EnvInfo {
    const char* name;
    int S, A, O, P, H, I, K;
    const char* pnames[MAXP];
    float nominal[MAXP];
    float des[MAXS], qd[MAXS], rd[MAXA];
};

// names/nominal values: get_nominal_domain_param of each env; task defaults: _create_task of each env
static const EnvInfo ENV_INFO[VS_ENV_COUNT] = {
    {"omo", Omo::S, Omo::A, Omo::O, Omo::P, Omo::H, Omo::I, Omo::K,
     {"mass", "stiffness", "damping"},
     {1.0f, 30.0f, 0.5f},  // one_mass_oscillator.py:82-86
     {0, 0}, {1e1f, 1e-2f}, {1e-6f}},  // :70-73
    {"bob", Bob::S, Bob::A, Bob::O, Bob::P, Bob::H, Bob::I, Bob::K,
     {"gravity_const", "ball_mass", "ball_radius", "beam_mass", "beam_length", "beam_thickness", "friction_coeff",
      "ang_offset"},
     {9.81f, 0.5f, 0.1f, 3.0f, 2.0f, 0.1f, 0.05f, 0.0f},  // ball_on_beam.py:77-87
     {0, 0, 0, 0}, {1e5f, 1e3f, 1e3f, 1e2f}, {1.0f}},  // :100-108
    {"qq-su", QQ::S, QQ::A, QQ::O, QQ::P, QQ::H, QQ::I, QQ::K,
     {"gravity_const", "motor_resistance", "motor_back_emf", "mass_rot_pole", "length_rot_pole", "damping_rot_pole",
      "mass_pend_pole", "length_pend_pole", "damping_pend_pole", "voltage_thold_neg", "voltage_thold_pos"},
     {9.81f, 8.4f, 0.042f, 0.095f, 0.085f, 5e-6f, 0.024f, 0.129f, 1e-6f, 0.0f, 0.0f},  // quanser_qube.py:54-68
     {0.0f, PI_F, 0.0f, 0.0f}, {1.0f, 1.0f, 2e-2f, 5e-3f}, {4e-3f}},  // :181-188
    {"qcp-su", Qcp::S, Qcp::A, Qcp::O, Qcp::P, Qcp::H, Qcp::I, Qcp::K,
     {"gravity_const", "cart_mass", "rail_length", "motor_efficiency", "gear_efficiency", "gear_ratio",
      "motor_inertia", "pinion_radius", "motor_resistance", "motor_back_emf", "pole_damping", "combined_damping",
      "pole_mass", "pole_length", "cart_friction_coeff", "voltage_thold_neg", "voltage_thold_pos"},
     {9.81f, 0.58f, 0.814f, 0.9f, 0.9f, 3.71f, 3.9e-7f, 6.35e-3f, 2.6f, 7.67e-3f, 0.0024f, 5.4f, 0.127f,
      0.3365f / 2, 0.02f, 0.0f, 0.0f},  // quanser_cartpole.py:111-143
     {0.0f, PI_F, 0.0f, 0.0f}, {3e-1f, 5e-1f, 5e-3f, 1e-3f}, {1e-3f}},  // :573-587
    {"qbb", Qbb::S, Qbb::A, Qbb::O, Qbb::P, Qbb::H, Qbb::I, Qbb::K,
     {"gravity_const", "ball_mass", "ball_radius", "plate_length", "arm_radius", "gear_ratio", "gear_efficiency",
      "load_inertia", "motor_inertia", "motor_back_emf", "motor_resistance", "motor_efficiency", "combined_damping",
      "ball_damping", "voltage_thold_x_pos", "voltage_thold_x_neg", "voltage_thold_y_pos", "voltage_thold_y_neg",
      "offset_th_x", "offset_th_y"},
     {9.81f, 0.003f, 0.019625f, 0.275f, 0.0254f, 70.0f, 0.9f, 5.2822e-5f, 4.6063e-7f, 0.0077f, 2.6f, 0.69f, 0.015f,
      0.05f, 0.28f, -0.10f, 0.28f, -0.074f, 0.0f, 0.0f},  // quanser_ball_balancer.py:141-143,171-202
     {0, 0, 0, 0, 0, 0, 0, 0}, {1e0f, 1e0f, 5e3f, 5e3f, 1e-2f, 1e-2f, 5e-1f, 5e-1f}, {1e-2f, 1e-2f}},  // :119-129
    // ---- the remaining pysim families ----
    {"qq-st", QQSt::S, QQSt::A, QQSt::O, QQSt::P, QQSt::H, QQSt::I, QQSt::K,
     {"gravity_const", "motor_resistance", "motor_back_emf", "mass_rot_pole", "length_rot_pole", "damping_rot_pole",
      "mass_pend_pole", "length_pend_pole", "damping_pend_pole", "voltage_thold_neg", "voltage_thold_pos"},
     {9.81f, 8.4f, 0.042f, 0.095f, 0.085f, 5e-6f, 0.024f, 0.129f, 1e-6f, 0.0f, 0.0f},
     {0.0f, PI_F, 0.0f, 0.0f}, {3.0f, 4.0f, 2.0f, 2.0f}, {5e-2f}},  // quanser_qube.py:215-222
    {"qcp-st", QcpSt::S, QcpSt::A, QcpSt::O, QcpSt::P, QcpSt::H, QcpSt::I, QcpSt::K,
     {"gravity_const", "cart_mass", "rail_length", "motor_efficiency", "gear_efficiency", "gear_ratio",
      "motor_inertia", "pinion_radius", "motor_resistance", "motor_back_emf", "pole_damping", "combined_damping",
      "pole_mass", "pole_length", "cart_friction_coeff", "voltage_thold_neg", "voltage_thold_pos"},
     {9.81f, 0.58f, 0.814f, 0.9f, 0.9f, 3.71f, 3.9e-7f, 6.35e-3f, 2.6f, 7.67e-3f, 0.0024f, 5.4f, 0.127f,
      0.3365f / 2, 0.02f, 0.0f, 0.0f},
     {0.0f, PI_F, 0.0f, 0.0f}, {5e-0f, 1e1f, 1e-2f, 1e-2f}, {1e-3f}},  // quanser_cartpole.py:494-504
    {"pend", Pend::S, Pend::A, Pend::O, Pend::P, Pend::H, Pend::I, Pend::K,
     {"gravity_const", "pole_mass", "pole_length", "pole_damping", "torque_thold"},
     {9.81f, 1.0f, 1.0f, 0.05f, 3.5f},  // pendulum.py:94-101
     {PI_F, 0.0f}, {1e-0f, 1e-3f}, {1e-2f}},  // :82-87
    {"bob-d", BobD::S, BobD::A, BobD::O, BobD::P, BobD::H, BobD::I, BobD::K,
     {"gravity_const", "ball_mass", "ball_radius", "beam_mass", "beam_length", "beam_thickness", "friction_coeff",
      "ang_offset"},
     {9.81f, 0.5f, 0.1f, 3.0f, 2.0f, 0.1f, 0.05f, 0.0f},
     {0, 0, 0, 0}, {1e5f, 1e3f, 1e3f, 1e2f}, {1.0f}}};

static thread_local std::string g_create_err;

static int fail(vs_handle h, int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else
        snprintf(buf, sizeof buf, "%s", what);
    if (h) h->err = buf;
    else g_create_err = buf;
    return code;
}

// ... with the entry point's name in front: shared checks word their refusals as the entry point itself would
static int fail(vs_handle h, int code, const char* who, const char* what, hipError_t e = hipSuccess) {
    return fail(h, code, (std::string(who) + ": " + what).c_str(), e);
}

#define HIPCHK(h, x)                                              \
    do {                                                          \
        hipError_t e_ = (x);                                      \
        if (e_ != hipSuccess) return fail(h, VS_ERR_HIP, #x, e_); \
    } while (0)

#define DISPATCH_ENV(type, ...)                                  \
    switch (type) {                                              \
        case VS_ENV_OMO: { using E = Omo; __VA_ARGS__; } break;    \
        case VS_ENV_BOB: { using E = Bob; __VA_ARGS__; } break;    \
        case VS_ENV_QQ_SU: { using E = QQ; __VA_ARGS__; } break;   \
        case VS_ENV_QCP_SU: { using E = Qcp; __VA_ARGS__; } break; \
        case VS_ENV_QBB: { using E = Qbb; __VA_ARGS__; } break;    \
        case VS_ENV_QQ_ST: { using E = QQSt; __VA_ARGS__; } break; \
        case VS_ENV_QCP_ST: { using E = QcpSt; __VA_ARGS__; } break; \
        case VS_ENV_PEND: { using E = Pend; __VA_ARGS__; } break;  \
        case VS_ENV_BOB_D: { using E = BobD; __VA_ARGS__; } break; \
        default: break;                                          \
    }

static bool is_device_ptr(const void* p) {
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // clear: plain host memory is reported as an error
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

template <class T>
static int dalloc(vs_handle h, T** p, size_t count) {
    void* q = nullptr;
    HIPCHK(h, hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 4));
    HIPCHK(h, hipMemsetAsync(q, 0, count * sizeof(T) > 0 ? count * sizeof(T) : 4, h->stream));
    h->allocs.push_back(q);
    *p = (T*)q;
    return VS_OK;
}

// free the device buffers that are set and forget them (not for members of h->allocs)
template <class T, class... Ts>
static int dfree(vs_handle h, T*& p, Ts*&... rest) {
    if (p) HIPCHK(h, hipFree((void*)p));
    p = nullptr;
    if constexpr (sizeof...(rest) > 0) return dfree(h, rest...);
    return VS_OK;
}

// stage a host SoA [rows][pitch] into device memory [rows][ld]; device inputs are used in place
static int stage_rows(vs_handle h, const float* src, int rows, int64_t pitch, const float** out, long* out_pitch) {
    if (is_device_ptr(src)) {
        *out = src;
        *out_pitch = (long)pitch;
        return VS_OK;
    }
    size_t need = (size_t)rows * h->d.ld * sizeof(float);
    if (need > h->stage_bytes) {
        if (h->stage) HIPCHK(h, hipFree(h->stage));
        h->stage = nullptr;
        h->stage_bytes = 0;
        HIPCHK(h, hipMalloc(&h->stage, need));
        h->stage_bytes = need;
    }
    HIPCHK(h, hipMemcpy2DAsync(h->stage, (size_t)h->d.ld * 4, src, (size_t)pitch * 4, (size_t)h->d.n * 4, rows,
                               hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // control path: the caller's host buffer may be a temporary
    *out = (const float*)h->stage;
    *out_pitch = h->d.ld;
    return VS_OK;
}

static int stage_mask(vs_handle h, const uint8_t* mask, const uint8_t** out) {
    if (!mask) { *out = nullptr; return VS_OK; }
    if (is_device_ptr(mask)) { *out = mask; return VS_OK; }
    if (!h->stage_mask) HIPCHK(h, hipMalloc(&h->stage_mask, (size_t)h->d.ld));
    HIPCHK(h, hipMemcpyAsync(h->stage_mask, mask, (size_t)h->d.n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *out = (const uint8_t*)h->stage_mask;
    return VS_OK;
}

static int check_specs(vs_handle h, const vs_dp_spec* specs, int n, DrSpecs* out) {
    const EnvInfo& ei = ENV_INFO[h->type];
    if (n < 0 || n > MAXP || (n > 0 && !specs)) return fail(h, VS_ERR_ARG, "bad domain-parameter spec list");
    out->n = n;
    for (int q = 0; q < n; ++q) {
        if (specs[q].param_index < 0 || specs[q].param_index >= ei.P) return fail(h, VS_ERR_ARG, "spec param_index out of range");
        const int kind = specs[q].kind;
        if (kind != VS_DP_NORMAL && kind != VS_DP_UNIFORM && kind != VS_DP_BERNOULLI) return fail(h, VS_ERR_ARG, "spec kind must be VS_DP_NORMAL, VS_DP_UNIFORM or VS_DP_BERNOULLI");
        if (kind != VS_DP_BERNOULLI && !(specs[q].spread >= 0.f)) return fail(h, VS_ERR_ARG, "spec spread must be >= 0");
        if (kind == VS_DP_BERNOULLI && !(specs[q].aux >= 0.f && specs[q].aux <= 1.f)) return fail(h, VS_ERR_ARG, "spec aux (prob_1) must be in [0, 1]");
        out->s[q] = specs[q];
    }
    return VS_OK;
}

struct vs_mixed {
    int n = 0;
    vs_handle sub[MAX_SEG]{};
    Segs host{};
    Segs* dev = nullptr;
    int total_blocks = 0;
    std::string err;
};

// some member redraws domain parameters at a reset inside the launch (live randomizer / parameter buffer)
static bool mixed_redraws(const vs_mixed* m) {
    for (int q = 0; q < m->n; ++q)
        if (m->sub[q]->d.dr_n > 0 || m->sub[q]->d.pbuf_n > 0) return true;
    return false;
}

// What every mixed launch checks before it touches a member: the members still agree on what the ONE launch takes from the
// first of them (auto-reset, the stream; for a rollout the record mode), none carries a wrapper pipeline, and a recording
// rollout fits every member's record buffers.  A refusal names the entry point (`who`) and leaves every handle as it was.
static int mixed_check(vs_mixed* m, const char* who, bool rollout, int k_steps, int record) {
    auto refuse = [&](const char* what) {
        m->err = std::string(who) + ": " + what;
        return VS_ERR_STATE;
    };
    vs_handle h0 = m->sub[0];
    for (int q = 0; q < m->n; ++q) {
        vs_handle h = m->sub[q];
        if (rollout && record && h->d.traj_t0 + k_steps > h->traj_cap) return refuse("k_steps exceeds a segment's vs_set_traj_capacity");
        if (h->auto_reset != h0->auto_reset) return refuse("segments differ in auto-reset");
        if (rollout && h->record_mode != h0->record_mode) return refuse("segments differ in record mode");
        if (h->d.pipe.act_on || h->d.pipe.obs_on)
            return refuse("a segment carries an action/observation pipeline (single-family handles only)");
        // one launch, one stream: a member moved to another one would no longer order its own resets and copies with the launch
        if (h->stream != h0->stream) return refuse("a segment's stream differs from the first segment's (vs_set_stream after vs_mixed_create)");
    }
    return VS_OK;
}

// the segment table of one launch (after mixed_check); the members' action streams advance once it is on the device
static int mixed_upload(vs_mixed* m, const float* const* acts, const int64_t* env_strides, const int64_t* dim_strides,
                        int k_steps) {
    int blocks = 0;
    vs_handle h0 = m->sub[0];
    for (int q = 0; q < m->n; ++q) {
        vs_handle h = m->sub[q];
        Seg& sg = m->host.s[q];
        blocks += (h->d.ld + BLOCK - 1) / BLOCK;
        sg.type = h->type;
        sg.block_end = blocks;
        sg.T = h->task;
        sg.d = h->d;
        sg.act = acts ? acts[q] : nullptr;
        sg.env_stride = env_strides ? (long)env_strides[q] : 0;
        sg.dim_stride = dim_strides ? (long)dim_strides[q] : 0;
        sg.reset_seed = h->ar_seed;
        sg.epoch0 = h->epoch;
    }
    m->host.n = m->n;
    m->total_blocks = blocks;
    // the segment table travels through device memory (kernel arguments are capped at 4 KB); hipMemcpyAsync from the
    // pageable host copy is ordered on the stream before the launch that reads it
    hipError_t e = hipMemcpyAsync(m->dev, &m->host, sizeof(Segs), hipMemcpyHostToDevice, h0->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h0->stream);  // host.s is rewritten by the next call
    if (e != hipSuccess) { m->err = std::string("mixed_upload: ") + hipGetErrorString(e); return VS_ERR_HIP; }
    for (int q = 0; q < m->n; ++q) m->sub[q]->epoch += (uint64_t)k_steps;
    return VS_OK;
}

// ---- the policy slot of a handle: one in-kernel policy at a time, shared by the setters of the four kinds and vs_destroy
static int drop_pop(vs_handle h) {
    if (int rc = dfree(h, h->pop.w, h->pop.wg_set, h->pp.ent, h->pp.wg, h->pp.seg)) return rc;
    h->pp.wg_host.clear();
    h->pp.t_steps = h->pp.n_wg = 0;
    h->pop = Pop{};
    h->pop_sets = 0;
    h->pop_g256 = h->pop_inert = false;
    return VS_OK;
}

static int drop_fnn(vs_handle h) {
    if (int rc = dfree(h, h->fnn.w)) return rc;
    h->fnn = Fnn{};
    return VS_OK;
}

static int drop_rnn(vs_handle h) {
    if (int rc = dfree(h, h->rnn.w, h->rnn.hid)) return rc;
    h->rnn = Rnn{};
    return VS_OK;
}

static int drop_lin(vs_handle h) {
    if (int rc = dfree(h, h->lin.w)) return rc;
    h->lin = Lin{};
    return VS_OK;
}

static int drop_sens(vs_handle h) {
    if (int rc = dfree(h, h->sens.grad, h->sens.gn, h->sens.sens)) return rc;
    h->sens = Sens{};
    return VS_OK;
}

static int drop_target(vs_handle h) {
    if (int rc = drop_sens(h)) return rc;  // (the sensitivities belong to the target's sum)
    return dfree(h, h->play.tgt, h->play.loss);
}

static int drop_play(vs_handle h) {  // the playback policy and the target that belongs to it
    if (int rc = drop_target(h)) return rc;
    if (int rc = dfree(h, h->play.act, h->play.rec_len, h->play.lane_rec)) return rc;
    h->play = Play{};
    return VS_OK;
}

// one in-kernel policy at a time: whichever kind is set goes, with what belongs to it -- the running hidden state, the playback
// target and its sensitivities, the population (it was set for this policy), the packer's index map and the workspace of the
// parameter-gradient pass (its index map and the width of its partial vectors are this policy's)
static int drop_policy(vs_handle h) {
    if (int rc = drop_fnn(h)) return rc;
    if (int rc = drop_rnn(h)) return rc;
    if (int rc = drop_lin(h)) return rc;
    if (int rc = drop_play(h)) return rc;
    if (int rc = drop_pop(h)) return rc;
    if (int rc = dfree(h, h->pg.part, h->pg.map, h->pg.npart, h->pg.nmap)) return rc;
    h->pg.wgs = h->pg.nwgs = 0;
    h->pol_map.clear();
    h->pol_n_params = 0;
    return VS_OK;
}

// The workspace for a grid of n_wg workgroups and partial vectors of psize floats.  It belongs to the policy on the handle
// (drop_policy frees it, so psize and the map are this policy's): the index map goes up on first use, the partial buffer grows when a
// grid is larger than every one before and never shrinks.
static int param_grad_workspace(vs_handle h, const char* who, int psize, int n_wg) {
    if (!h->pg.map) {
        int* map = nullptr;
        HIPCHK(h, hipMalloc((void**)&map, (size_t)psize * sizeof(int)));
        hipError_t e = hipMemcpy(map, h->pol_map.data(), (size_t)psize * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(map); return fail(h, VS_ERR_HIP, who, "index map upload", e); }
        h->pg.map = map;
    }
    if (n_wg > h->pg.wgs) {
        if (h->pg.part) HIPCHK(h, hipStreamSynchronize(h->stream));  // (an earlier call may still read the smaller one)
        if (int rc = dfree(h, h->pg.part)) return rc;
        h->pg.wgs = 0;
        HIPCHK(h, hipMalloc((void**)&h->pg.part, (size_t)n_wg * psize * sizeof(float)));
        h->pg.wgs = n_wg;
    }
    return VS_OK;
}

// the reduction of the n_wg partial vectors into d_params, in parameters_to_vector's order
static void launch_param_reduce(vs_handle h, int n_wg, int psize, float* d_params, int accumulate) {
    hipLaunchKernelGGL((k_fnn_param_reduce<4>), dim3((unsigned)((psize + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, h->stream,
                       (const float*)h->pg.part, n_wg, psize, (const int*)h->pg.map, d_params, accumulate != 0 ? 1 : 0);
}

// the observation rows a policy sees, descriptor D -> kernel arguments P (n_obs == 0: all of them, in order; ident: exactly that)
template <class D, class P>
static int policy_view(vs_handle h, const char* who, const D& desc, P& f) {
    const int O = ENV_INFO[h->type].O;
    f.n_vis = desc.n_obs > 0 ? desc.n_obs : O;
    if (f.n_vis > O) return fail(h, VS_ERR_ARG, who, "more visible observation rows than the env has");
    f.ident = f.n_vis == O;
    for (int k = 0; k < f.n_vis; ++k) {
        f.obs_idx[k] = desc.n_obs > 0 ? desc.obs_idx[k] : k;
        if (f.obs_idx[k] < 0 || f.obs_idx[k] >= O) return fail(h, VS_ERR_ARG, who, "obs_idx out of range");
        if (f.obs_idx[k] != k) f.ident = 0;
    }
    return VS_OK;
}

// ... and its exploration noise
template <class D, class P>
static int policy_noise(vs_handle h, const char* who, const D& desc, P& f) {
    for (int j = 0; j < ENV_INFO[h->type].A; ++j) {
        f.noise_std[j] = desc.noise_std[j];
        if (!(f.noise_std[j] >= 0.f)) return fail(h, VS_ERR_ARG, who, "noise_std must be >= 0");
        if (f.noise_std[j] > 0.f) f.noisy = 1;
    }
    return VS_OK;
}

// the packed vector of one policy in a new device buffer: the caller's `need` parameters (host or device) laid out by the
// index map (packed slot -> source index, -1: zero padding)
static int upload_packed(vs_handle h, const char* who, const std::vector<int>& map, const float* params, int64_t need, const float** out) {
    std::vector<float> src((size_t)need), pk(map.size(), 0.f);
    HIPCHK(h, hipMemcpy(src.data(), params, (size_t)need * sizeof(float), is_device_ptr(params) ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
    for (size_t q = 0; q < map.size(); ++q)
        if (map[q] >= 0) pk[q] = src[(size_t)map[q]];
    float* dw = nullptr;
    HIPCHK(h, hipMalloc((void**)&dw, pk.size() * sizeof(float)));
    hipError_t e = hipMemcpy(dw, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dw); return fail(h, VS_ERR_HIP, who, "upload", e); }
    *out = dw;
    return VS_OK;
}

extern "C" {

int vs_version(void) { return 321; }

static int record_width(int t, int mode) {
    const EnvInfo& e = ENV_INFO[t];
    return mode == 2 ? e.O + e.A + 1 + e.S + e.A + e.H : e.O + e.A + 1;
}

int vs_traj_layout(int t, int mode, int* F, int* nq, int* h2, int* h1) {
    if (t < 0 || t >= VS_ENV_COUNT || mode < 1 || mode > 2) return VS_ERR_ARG;
    const int f = record_width(t, mode);
    if (F) *F = f;
    if (nq) *nq = f / 4;
    if (h2) *h2 = (f % 4) >= 2 ? 1 : 0;
    if (h1) *h1 = f % 2;
    return VS_OK;
}

int vs_env_dims(int t, int* S, int* A, int* O, int* P, int* H, int* I, int* K) {
    if (t < 0 || t >= VS_ENV_COUNT) return VS_ERR_ARG;
    const EnvInfo& e = ENV_INFO[t];
    if (S) *S = e.S;
    if (A) *A = e.A;
    if (O) *O = e.O;
    if (P) *P = e.P;
    if (H) *H = e.H;
    if (I) *I = e.I;
    if (K) *K = e.K;
    return VS_OK;
}

const char* vs_env_name(int t) { return (t < 0 || t >= VS_ENV_COUNT) ? nullptr : ENV_INFO[t].name; }

const char* vs_param_name(int t, int i) {
    if (t < 0 || t >= VS_ENV_COUNT || i < 0 || i >= ENV_INFO[t].P) return nullptr;
    return ENV_INFO[t].pnames[i];
}

int vs_nominal_params(int t, int flags, float* out) {
    if (t < 0 || t >= VS_ENV_COUNT || !out) return VS_ERR_ARG;
    for (int k = 0; k < ENV_INFO[t].P; ++k) out[k] = ENV_INFO[t].nominal[k];
    if ((t == VS_ENV_QCP_SU || t == VS_ENV_QCP_ST) && (flags & VS_FLAG_LONG_POLE)) {  // get_nominal_domain_param(long=True), :113-118
        out[12] = 0.23f;
        out[13] = 0.641f / 2;
    }
    return VS_OK;
}

const char* vs_last_error(vs_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int vs_create(int env_type, int64_t n_envs, double dt, int64_t max_steps, int device_id, const vs_task_cfg* cfg,
              vs_handle* out) {
    if (!out) return fail(nullptr, VS_ERR_ARG, "vs_create: out is NULL");
    *out = nullptr;
    if (env_type < 0 || env_type >= VS_ENV_COUNT) return fail(nullptr, VS_ERR_ARG, "vs_create: unknown env_type");
    if (n_envs < 1 || n_envs > (1LL << 30)) return fail(nullptr, VS_ERR_ARG, "vs_create: n_envs must be in [1, 2^30]");
    if (!(dt >= 0.0)) return fail(nullptr, VS_ERR_ARG, "vs_create: dt must be >= 0");  // Env.__init__ base.py:58-59
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(nullptr, VS_ERR_HIP, "vs_create: no HIP device available (libvecsim has no CPU fallback)", e);
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, VS_ERR_ARG, "vs_create: bad device_id");
    vs_handle h = new (std::nothrow) vs_env();
    if (!h) return fail(nullptr, VS_ERR_HIP, "vs_create: out of host memory");
    h->type = env_type;
    h->device = device_id;
    {
        int cu = 0;
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cu > 0) h->n_cu = cu;
    }
    const EnvInfo& ei = ENV_INFO[env_type];
    Task& T = h->task;
    bool defaults = !cfg || cfg->use_defaults;
    for (int j = 0; j < MAXS; ++j) {
        T.des[j] = defaults ? ei.des[j] : cfg->state_des[j];
        T.qd[j] = defaults ? ei.qd[j] : cfg->q_diag[j];
    }
    for (int j = 0; j < MAXA; ++j) T.rd[j] = defaults ? ei.rd[j] : cfg->r_diag[j];
    T.dt = (float)dt;
    T.max_steps = (max_steps <= 0 || max_steps >= INT_MAX) ? INT_MAX : (int)max_steps;
    // without a cfg the ctor defaults of the reference apply: QCartPoleStabSim(long=True, simple_dynamics=True)
    T.flags = cfg ? cfg->flags : (env_type == VS_ENV_QCP_ST ? (VS_FLAG_LONG_POLE | VS_FLAG_SIMPLE_DYNAMICS) : 0);
    T.wild_init = cfg ? cfg->wild_init : 0;
    for (int j = 0; j < MAXS; ++j) T.init_fixed[j] = cfg ? cfg->init_state[j] : 0.f;
    int rc = VS_OK;
#define CK(x) do { rc = (x); if (rc != VS_OK) { g_create_err = h->err; vs_destroy(h); return rc; } } while (0)
#define HK(x) do { hipError_t e2 = (x); if (e2 != hipSuccess) { fail(nullptr, VS_ERR_HIP, #x, e2); vs_destroy(h); return VS_ERR_HIP; } } while (0)
    HK(hipSetDevice(device_id));
    // a BLOCKING stream: it orders itself with the legacy default stream, which is where torch (and most callers) run
    // unless told otherwise -- zero-copy views of the handle's buffers can then be read by default-stream work without
    // an explicit sync.  Callers on other non-blocking streams hand theirs over with vs_set_stream.
    HK(hipStreamCreateWithFlags(&h->own_stream, hipStreamDefault));
    h->stream = h->own_stream;
    Dev& d = h->d;
    d.n = (int)n_envs;
    d.ld = (int)(((n_envs + BLOCK - 1) / BLOCK) * BLOCK);
    size_t ld = d.ld;
    CK(dalloc(h, &d.state, ei.S * ld));
    CK(dalloc(h, &d.hidden, (ei.H > 0 ? ei.H : 1) * ld));
    CK(dalloc(h, &d.obs, ei.O * ld));
    CK(dalloc(h, &d.rew, ld));
    CK(dalloc(h, &d.ret, ld));
    CK(dalloc(h, &d.consts, ei.K * ld));
    CK(dalloc(h, &d.params, ei.P * ld));
    CK(dalloc(h, &d.consts_uni, (size_t)MAXK));
    CK(dalloc(h, &d.done, ld));
    CK(dalloc(h, &d.failed, ld));
    CK(dalloc(h, &d.err, ld));
    CK(dalloc(h, &d.yielded, ld));
    CK(dalloc(h, &d.step, ld));
    CK(dalloc(h, &d.ep_idx, ld));
    CK(dalloc(h, &d.es_count, ld));
    CK(dalloc(h, &d.es_retsum, ld));
    CK(dalloc(h, &d.es_lensum, ld));
    CK(dalloc(h, &h->d_specs, (size_t)1));
    d.ep_cap = (unsigned)(ld < (1u << 16) ? (1u << 16) : ld);
    CK(dalloc(h, &d.ep_ret, (size_t)d.ep_cap));
    CK(dalloc(h, &d.ep_len, (size_t)d.ep_cap));
    CK(dalloc(h, &d.ep_env, (size_t)d.ep_cap));
    CK(dalloc(h, &d.ep_count, (size_t)1));
    CK(dalloc(h, &h->d_counter, (size_t)1));
    CK(dalloc(h, &d.rec_row, (size_t)1));
#ifdef VS_WS_STAMP
    CK(dalloc(h, &d.dbg, (size_t)(ld / 64) * 12));
#endif

    float nominal[MAXP];
    vs_nominal_params(env_type, T.flags, nominal);
    CK(vs_set_params_uniform(h, nominal));
    CK(vs_reset(h, nullptr, 0, 0, nullptr, 0));
    HK(hipStreamSynchronize(h->stream));
#undef CK
#undef HK
    *out = h;
    return VS_OK;
}

int vs_destroy(vs_handle h) {
    if (!h) return VS_OK;
    (void)hipSetDevice(h->device);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->stage) (void)hipFree(h->stage);
    if (h->stage_mask) (void)hipFree(h->stage_mask);
    if (h->d_pbuf) (void)hipFree(h->d_pbuf);
    if (h->d_ring) (void)hipFree(h->d_ring);
    (void)drop_policy(h);
    if (h->d_hrec) (void)hipFree(h->d_hrec);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return VS_OK;
}

int vs_set_stream(vs_handle h, void* s) {
    if (!h) return VS_ERR_ARG;
    // the caller orders work across streams (events / torch stream semantics); a capturing stream must not be synced
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &st) != hipSuccess) (void)hipGetLastError();
    if (st == hipStreamCaptureStatusNone) HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream = s ? (hipStream_t)s : h->own_stream;
    return VS_OK;
}

int vs_sync(vs_handle h) {
    if (!h) return VS_ERR_ARG;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VS_OK;
}

int64_t vs_n_envs(vs_handle h) { return h ? h->d.n : -1; }
int64_t vs_ld(vs_handle h) { return h ? h->d.ld : -1; }

int vs_set_params(vs_handle h, const float* params_soa, int64_t pitch, const uint8_t* mask) {
    if (!h || !params_soa) return fail(h, VS_ERR_ARG, "vs_set_params: NULL argument");
    if (pitch < h->d.n) return fail(h, VS_ERR_ARG, "vs_set_params: pitch < n_envs");
    HIPCHK(h, hipSetDevice(h->device));
    const float* src; long sp; const uint8_t* m;
    int rc = stage_rows(h, params_soa, ENV_INFO[h->type].P, pitch, &src, &sp);
    if (rc) return rc;
    rc = stage_mask(h, mask, &m);
    if (rc) return rc;
    h->uniform = false;
    DISPATCH_ENV(h->type, Launch<E>::set_params(h, src, sp, 0, m));
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_set_params_uniform(vs_handle h, const float* params) {
    if (!h || !params) return fail(h, VS_ERR_ARG, "vs_set_params_uniform: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    int P = ENV_INFO[h->type].P;
    if (h->stage_bytes < (size_t)MAXP * 4) {
        if (h->stage) HIPCHK(h, hipFree(h->stage));
        h->stage_bytes = 0;
        HIPCHK(h, hipMalloc(&h->stage, (size_t)MAXP * 4));
        h->stage_bytes = (size_t)MAXP * 4;
    }
    HIPCHK(h, hipMemcpyAsync(h->stage, params, (size_t)P * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // `params` may be a temporary of the caller
    h->uniform = true;
    DISPATCH_ENV(h->type, Launch<E>::set_params(h, (const float*)h->stage, 0L, 1, (const uint8_t*)nullptr));
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_sample_params(vs_handle h, const vs_dp_spec* specs, int n_specs, uint64_t seed, const uint8_t* mask) {
    if (!h) return VS_ERR_ARG;
    DrSpecs dr;
    int rc = check_specs(h, specs, n_specs, &dr);
    if (rc) return rc;
    if (n_specs == 0) return VS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const uint8_t* m;
    rc = stage_mask(h, mask, &m);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_specs, &dr, sizeof(DrSpecs), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // `dr` lives on this stack frame
    h->uniform = false;
    DISPATCH_ENV(h->type, Launch<E>::sample_params(h, seed, m));
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_set_randomizer(vs_handle h, const vs_dp_spec* specs, int n_specs) {
    if (!h) return VS_ERR_ARG;
    DrSpecs dr;
    int rc = check_specs(h, specs, n_specs, &dr);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (dr.n > 0 && h->d.pbuf_n > 0) return fail(h, VS_ERR_STATE, "vs_set_randomizer: a parameter buffer is set");
    h->dr = dr;
    h->d.drv = dr;  // travels with every launch as part of the kernel arguments
    h->d.dr_n = dr.n;
    if (n_specs > 0) h->uniform = false;
    return VS_OK;
}

int vs_set_param_buffer(vs_handle h, const float* params_soa, int n_sets, int selection) {
    if (!h || n_sets < 0 || (n_sets > 0 && !params_soa) || selection < 0 || selection > 1)
        return fail(h, VS_ERR_ARG, "vs_set_param_buffer: bad argument");
    if (n_sets > 0 && h->dr.n > 0) return fail(h, VS_ERR_STATE, "vs_set_param_buffer: a live randomizer is set");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->d_pbuf) { HIPCHK(h, hipFree(h->d_pbuf)); h->d_pbuf = nullptr; }
    h->d.pbuf = nullptr;
    h->d.pbuf_n = 0;
    h->d.pbuf_mode = selection;
    if (n_sets == 0) return VS_OK;
    size_t bytes = (size_t)ENV_INFO[h->type].P * n_sets * sizeof(float);
    HIPCHK(h, hipMalloc((void**)&h->d_pbuf, bytes));
    HIPCHK(h, hipMemcpy(h->d_pbuf, params_soa, bytes, hipMemcpyHostToDevice));
    h->d.pbuf = h->d_pbuf;
    h->d.pbuf_n = n_sets;
    h->uniform = false;
    return VS_OK;
}

int vs_set_act_norm(vs_handle h, int on) {
    if (!h) return VS_ERR_ARG;
    if (on) h->task.flags |= VS_FLAG_ACT_NORM;
    else h->task.flags &= ~VS_FLAG_ACT_NORM;
    return VS_OK;
}

int vs_set_act_pipeline(vs_handle h, int delay, const float* noise_mean, const float* noise_std, int noise_normed,
                        int noise_after_delay, uint64_t seed) {
    if (!h) return VS_ERR_ARG;
    if (delay < 0 || delay > VS_MAX_ACT_DELAY) return fail(h, VS_ERR_ARG, "vs_set_act_pipeline: delay must be in [0, VS_MAX_ACT_DELAY]");
    const EnvInfo& ei = ENV_INFO[h->type];
    Pipe& p = h->d.pipe;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (delay != p.delay) {
        if (h->d_ring) { HIPCHK(h, hipFree(h->d_ring)); h->d_ring = nullptr; }
        if (delay > 0) {
            size_t bytes = (size_t)delay * ei.A * h->d.ld * sizeof(float);
            HIPCHK(h, hipMalloc((void**)&h->d_ring, bytes));
            // on the handle's stream: a null-stream memset is not ordered with kernels on a non-blocking stream
            HIPCHK(h, hipMemsetAsync(h->d_ring, 0, bytes, h->stream));
        }
        p.ring = h->d_ring;
        p.delay = delay;
    }
    p.act_noise = 0;
    for (int j = 0; j < MAXA; ++j) {
        p.a_mean[j] = (noise_mean && j < ei.A) ? noise_mean[j] : 0.f;
        p.a_std[j] = (noise_std && j < ei.A) ? noise_std[j] : 0.f;
        if (p.a_std[j] < 0.f || p.a_std[j] != p.a_std[j]) return fail(h, VS_ERR_ARG, "vs_set_act_pipeline: noise_std must be >= 0");
        if (p.a_mean[j] != 0.f || p.a_std[j] != 0.f) p.act_noise = 1;
    }
    p.noise_normed = noise_normed != 0;
    p.noise_after_delay = noise_after_delay != 0;
    p.seed = seed;
    p.act_on = p.delay > 0 || p.act_noise;
    return VS_OK;
}

int vs_set_obs_pipeline(vs_handle h, const float* scale, const float* shift, const float* noise_std, uint64_t seed) {
    if (!h) return VS_ERR_ARG;
    const EnvInfo& ei = ENV_INFO[h->type];
    Pipe& p = h->d.pipe;
    p.obs_noise = 0;
    bool ident = true;
    for (int j = 0; j < MAXO; ++j) {
        p.o_scale[j] = (scale && j < ei.O) ? scale[j] : 1.f;
        p.o_shift[j] = (shift && j < ei.O) ? shift[j] : 0.f;
        p.o_std[j] = (noise_std && j < ei.O) ? noise_std[j] : 0.f;
        if (p.o_std[j] < 0.f || p.o_std[j] != p.o_std[j]) return fail(h, VS_ERR_ARG, "vs_set_obs_pipeline: noise_std must be >= 0");
        if (p.o_std[j] != 0.f) p.obs_noise = 1;
        if (p.o_scale[j] != 1.f || p.o_shift[j] != 0.f) ident = false;
    }
    p.seed = seed;
    p.obs_on = !ident || p.obs_noise;
    // VS_OBS is the wrapped observation from now on
    HIPCHK(h, hipSetDevice(h->device));
    DISPATCH_ENV(h->type, Launch<E>::observe(h));
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

// rows of VS_ROLLOUT_GRAD / _GN / _SENS of a handle with sensitivities on
static void sens_rows(vs_handle h, int* g, int* t, int* s) {
    const EnvInfo& ei = ENV_INFO[h->type];
    *g = h->sens.n;
    *t = h->sens.n * (h->sens.n + 1) / 2;
    *s = (ei.S + ei.H) * h->sens.np;
}

// zero the three sensitivity buffers: every lane (m == nullptr) or the masked ones (m: the staged device mask)
static int zero_sens(vs_handle h, const uint8_t* m) {
    int rows[3];
    sens_rows(h, &rows[0], &rows[1], &rows[2]);
    float* bufs[3] = {h->sens.grad, h->sens.gn, h->sens.sens};
    for (int b = 0; b < 3; ++b) {
        if (!m) HIPCHK(h, hipMemsetAsync(bufs[b], 0, (size_t)rows[b] * h->d.ld * sizeof(float), h->stream));
        else hipLaunchKernelGGL(k_zero_rows_masked, grid_for(h->d.ld), dim3(BLOCK), 0, h->stream, bufs[b], rows[b], (size_t)h->d.ld, m, h->d.n);
    }
    return VS_OK;
}

int vs_reset(vs_handle h, const float* init_state, int64_t pitch, int full, const uint8_t* mask, uint64_t seed) {
    if (!h) return VS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const EnvInfo& ei = ENV_INFO[h->type];
    const float* src = nullptr; long sp = 0; const uint8_t* m;
    int rc;
    if (init_state) {
        if (pitch < h->d.n) return fail(h, VS_ERR_ARG, "vs_reset: pitch < n_envs");
        rc = stage_rows(h, init_state, full ? ei.S : ei.I, pitch, &src, &sp);
        if (rc) return rc;
    }
    rc = stage_mask(h, mask, &m);
    if (rc) return rc;
    DISPATCH_ENV(h->type, Launch<E>::reset(h, src, sp, full, m, seed));
    if (h->rnn.hid) {  // a new rollout starts from init_hidden()
        if (!m) HIPCHK(h, hipMemsetAsync(h->rnn.hid, 0, (size_t)h->rnn.hs * h->d.ld * sizeof(float), h->stream));
        else hipLaunchKernelGGL(k_zero_hidden, grid_for(h->d.ld), dim3(BLOCK), 0, h->stream, h->rnn.hid, h->rnn.hs, (size_t)h->d.ld, m, h->d.n);
    }
    if (h->play.loss) {  // a new rollout starts its discrepancy sum at 0
        if (!m) HIPCHK(h, hipMemsetAsync(h->play.loss, 0, (size_t)h->d.ld * sizeof(float), h->stream));
        else hipLaunchKernelGGL(k_zero_masked, grid_for(h->d.ld), dim3(BLOCK), 0, h->stream, h->play.loss, m, h->d.n);
    }
    if (h->sens.n) {  // ... and its sensitivities
        if (int rc2 = zero_sens(h, m)) return rc2;
    }
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_set_max_steps(vs_handle h, int64_t max_steps) {
    if (!h) return VS_ERR_ARG;
    h->task.max_steps = (max_steps <= 0 || max_steps >= INT_MAX) ? INT_MAX : (int)max_steps;
    return VS_OK;
}

int vs_set_dt(vs_handle h, double dt) {
    if (!h) return VS_ERR_ARG;
    if (!(dt >= 0.0)) return fail(h, VS_ERR_ARG, "vs_set_dt: dt must be >= 0");
    h->task.dt = (float)dt;  // no derived constant depends on the step size
    return VS_OK;
}

int vs_set_index_offset(vs_handle h, uint32_t first_global_index) {
    if (!h) return VS_ERR_ARG;
    h->d.idx0 = first_global_index;
    return VS_OK;
}

int vs_set_auto_reset(vs_handle h, int on, uint64_t seed) {
    if (!h) return VS_ERR_ARG;
    h->auto_reset = on != 0;
    h->ar_seed = seed;
    return VS_OK;
}

int vs_step(vs_handle h, const float* actions, int64_t env_stride, int64_t dim_stride) {
    if (!h || !actions) return fail(h, VS_ERR_ARG, "vs_step: NULL argument");
    // while the stream is being captured into a hipGraph only the launch itself may be issued (pointer queries and
    // device switches invalidate the capture); the pointer was validated by the eager warm-up call
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &st) != hipSuccess) (void)hipGetLastError();
    if (st == hipStreamCaptureStatusNone) {
        if (!is_device_ptr(actions)) return fail(h, VS_ERR_ARG, "vs_step: actions must be device memory");
        HIPCHK(h, hipSetDevice(h->device));
    }
    DISPATCH_ENV(h->type, Launch<E>::step(h, actions, (long)env_stride, (long)dim_stride));
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_step_record(vs_handle h, const float* actions, int64_t env_stride, int64_t dim_stride, int row) {
    if (!h || !actions) return fail(h, VS_ERR_ARG, "vs_step_record: NULL argument");
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &st) != hipSuccess) (void)hipGetLastError();
    if (st == hipStreamCaptureStatusNone) {
        if (!is_device_ptr(actions)) return fail(h, VS_ERR_ARG, "vs_step_record: actions must be device memory");
        HIPCHK(h, hipSetDevice(h->device));
    }
    if (h->traj_cap <= 0) return fail(h, VS_ERR_STATE, "vs_step_record: set the record capacity first (vs_set_traj_capacity)");
    if (row >= h->traj_cap) return fail(h, VS_ERR_STATE, "vs_step_record: row exceeds vs_set_traj_capacity");
    DISPATCH_ENV(h->type, Launch<E>::step(h, actions, (long)env_stride, (long)dim_stride, h->record_mode, row < 0 ? -1 : row));
    if (row < 0) hipLaunchKernelGGL(k_bump_row, dim3(1), dim3(1), 0, h->stream, h->d.rec_row);
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_set_record_row(vs_handle h, int row) {
    if (!h || row < 0) return fail(h, VS_ERR_ARG, "vs_set_record_row: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->d.rec_row, &row, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // `row` lives on this stack frame
    return VS_OK;
}

int vs_seek_random(vs_handle h, uint64_t step_index) {
    if (!h) return VS_ERR_ARG;
    h->epoch = step_index;
    return VS_OK;
}

int vs_step_jac(vs_handle h, const float* actions, int64_t env_stride, int64_t dim_stride) {
    if (!h || !actions) return fail(h, VS_ERR_ARG, "vs_step_jac: NULL argument");
    if (!is_device_ptr(actions)) return fail(h, VS_ERR_ARG, "vs_step_jac: actions must be device memory");
    if (h->auto_reset) return fail(h, VS_ERR_STATE, "vs_step_jac: switch auto-reset off (the Jacobian of a reset is meaningless)");
    if (h->d.pipe.act_on || h->d.pipe.obs_on)
        return fail(h, VS_ERR_STATE, "vs_step_jac: remove the action/observation pipeline (Jacobians are those of the bare env)");
    HIPCHK(h, hipSetDevice(h->device));
    const EnvInfo& ei = ENV_INFO[h->type];
    if (!h->d.jac_s) {
        size_t ni = (size_t)(ei.S + ei.A), ld = h->d.ld;
        int rc;
        if ((rc = dalloc(h, &h->d.jac_s, ei.S * ni * ld))) return rc;
        if ((rc = dalloc(h, &h->d.jac_r, ni * ld))) return rc;
        if ((rc = dalloc(h, &h->d.jac_o, ei.O * ni * ld))) return rc;
    }
    DISPATCH_ENV(h->type, Launch<E>::jac(h, actions, (long)env_stride, (long)dim_stride));
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

// the hidden-state record plane: traj_cap rows of hrec_width floats per env (when both are set)
static int alloc_hrec(vs_handle h) {
    if (int rc = dfree(h, h->d_hrec)) return rc;
    if (h->hrec_width <= 0 || h->traj_cap <= 0) return VS_OK;
    const size_t bytes = (size_t)h->traj_cap * h->hrec_width * h->d.ld * sizeof(float);
    HIPCHK(h, hipMalloc((void**)&h->d_hrec, bytes));
    HIPCHK(h, hipMemsetAsync(h->d_hrec, 0, bytes, h->stream));
    return VS_OK;
}

// the record buffers of a superseded capacity / mode are released at once (a sampler that resizes per call must not grow)
static int free_traj(vs_handle h) {
    Dev& d = h->d;
    void* old[2] = {d.traj_rec, d.traj_done};
    for (void* q : old) {
        if (!q) continue;
        for (size_t k = 0; k < h->allocs.size(); ++k)
            if (h->allocs[k] == q) { h->allocs.erase(h->allocs.begin() + (long)k); break; }
        HIPCHK(h, hipFree(q));
    }
    d.traj_rec = nullptr;
    d.traj_done = nullptr;
    if (int rc = dfree(h, h->d_hrec)) return rc;
    h->traj_cap = 0;
    d.traj_rows = 0;
    return VS_OK;
}

int vs_set_traj_capacity(vs_handle h, int t_max) {
    if (!h || t_max < 0) return fail(h, VS_ERR_ARG, "vs_set_traj_capacity: bad argument");
    if (t_max <= h->traj_cap) return VS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    Dev& d = h->d;
    size_t ld = d.ld;
    int rc;
    if ((rc = free_traj(h))) return rc;
    if ((rc = dalloc(h, &d.traj_rec, (size_t)t_max * record_width(h->type, h->record_mode) * ld))) return rc;
    if ((rc = dalloc(h, &d.traj_done, (size_t)((t_max + 31) / 32) * ld))) return rc;
    h->traj_cap = t_max;
    d.traj_rows = t_max;
    return alloc_hrec(h);
}

int vs_set_record_mode(vs_handle h, int mode) {
    if (!h || mode < 1 || mode > 2) return fail(h, VS_ERR_ARG, "vs_set_record_mode: 1 (obs | act | rew) or 2 (+ state | act_app | hidden)");
    if (mode == h->record_mode) return VS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int rc = free_traj(h);  // the row width changes: the capacity has to be set again
    if (rc) return rc;
    h->record_mode = mode;
    h->d.traj_t0 = 0;
    return VS_OK;
}

int vs_record_mode(vs_handle h) { return h ? h->record_mode : VS_ERR_ARG; }

int vs_set_freeze_done(vs_handle h, int on) {
    if (!h) return VS_ERR_ARG;
    if (on) h->task.flags |= VS_FLAG_FREEZE_DONE;
    else h->task.flags &= ~VS_FLAG_FREEZE_DONE;
    return VS_OK;
}

int vs_set_lean_step(vs_handle h, int on) {
    if (!h) return VS_ERR_ARG;
    if (on) h->task.flags |= VS_FLAG_LEAN_STEP;
    else h->task.flags &= ~VS_FLAG_LEAN_STEP;
    return VS_OK;
}

int vs_set_rollout_variant(vs_handle h, int variant) {
    if (!h || variant < -1 || variant > 4) return fail(h, VS_ERR_ARG, "vs_set_rollout_variant: -1 (automatic) or 0 .. 4");
    h->rollout_variant = variant;
    return VS_OK;
}

int vs_set_policy_shape(vs_handle h, int shape) {
    if (!h || shape < -1 || shape > 2) return fail(h, VS_ERR_ARG, "vs_set_policy_shape: -1 (automatic) or 0 .. 2");
    h->policy_shape = shape;
    return VS_OK;
}

int vs_rollout_variant(vs_handle h) {
    if (!h) return VS_ERR_ARG;
    int var = 0;
    DISPATCH_ENV(h->type, var = Launch<E>::variant(h));
    return var;
}

int vs_set_traj_offset(vs_handle h, int t0) {
    if (!h || t0 < 0) return fail(h, VS_ERR_ARG, "vs_set_traj_offset: bad argument");
    h->d.traj_t0 = t0;
    return VS_OK;
}

int vs_step_random(vs_handle h, uint64_t seed, int k_steps, int record) {
    if (!h || k_steps < 1) return fail(h, VS_ERR_ARG, "vs_step_random: bad argument");
    if (record && h->d.traj_t0 + k_steps > h->traj_cap) return fail(h, VS_ERR_STATE, "vs_step_random: traj offset + k_steps exceeds vs_set_traj_capacity");
    HIPCHK(h, hipSetDevice(h->device));
    uint64_t ep = h->epoch;
    h->epoch += (uint64_t)k_steps;
    DISPATCH_ENV(h->type, Launch<E>::rollout(h, k_steps, seed, ep, record ? h->record_mode : 0));
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_set_policy_fnn(vs_handle h, const vs_fnn_desc* desc, const float* params, int64_t n_params) {
    if (!h) return VS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (int rc = drop_policy(h)) return rc;  // before any check: a refused call leaves no policy
    if (!desc) return VS_OK;
    const EnvInfo& ei = ENV_INFO[h->type];
    const char* who = "vs_set_policy_fnn";
    if (h->type == VS_ENV_BOB_D) return fail(h, VS_ERR_ARG, "vs_set_policy_fnn: the discrete-action family takes no network policy");
    if (!params || desc->n_hidden < 1 || desc->n_hidden > FNN_MAXH) return fail(h, VS_ERR_ARG, "vs_set_policy_fnn: 1 .. 4 hidden layers and a parameter vector");
    Fnn f{};
    f.n_hidden = desc->n_hidden;
    if (int rc = policy_view(h, who, *desc, f)) return rc;
    f.feat = desc->feat != 0;
    if (f.feat && f.n_vis < 2) return fail(h, VS_ERR_ARG, "vs_set_policy_fnn: the sin / cos featurisation needs two observation rows");
    f.in_dim = f.n_vis + f.feat;
    f.out_dim = ei.A;
    f.out_nonlin = desc->output_nonlin;
    int64_t need = 0;
    int off = 0, last = f.in_dim;
    for (int l = 0; l < f.n_hidden; ++l) {
        f.hidden[l] = desc->hidden[l];
        f.hid_nonlin[l] = desc->hidden_nonlin[l];
        if (f.hidden[l] < 1 || f.hidden[l] > FNN_W) return fail(h, VS_ERR_ARG, "vs_set_policy_fnn: hidden layers are 1 .. 64 units wide");
        if (f.hid_nonlin[l] < 0 || f.hid_nonlin[l] > FNN_SIGMOID) return fail(h, VS_ERR_ARG, "vs_set_policy_fnn: unknown nonlinearity");
        need += (int64_t)f.hidden[l] * last + f.hidden[l];
        f.off_w[l] = off;
        off += (l == 0 ? last : FNN_W) * FNN_W;  // layers behind the first read all 64 (zero-padded) input rows
        f.off_b[l] = off;
        off += FNN_W;
        last = f.hidden[l];
    }
    if (f.out_nonlin < 0 || f.out_nonlin > FNN_SIGMOID) return fail(h, VS_ERR_ARG, "vs_set_policy_fnn: unknown nonlinearity");
    need += (int64_t)ei.A * last + ei.A;
    f.off_w[f.n_hidden] = off;
    off += ei.A * FNN_W;
    f.off_b[f.n_hidden] = off;
    off += 8;
    if (n_params != need) return fail(h, VS_ERR_ARG, "vs_set_policy_fnn: parameter count does not match the layer sizes");
    if (int rc = policy_noise(h, who, *desc, f)) return rc;
    // torch layout -> transposed, zero-padded rows: unit j of layer l reads Wt_l[k][j], contiguous over j (scalar-load friendly);
    // built as an index map (packed slot -> source index) that vs_set_policy_population reuses on the device
    std::vector<int> map((size_t)off, -1);
    int q = 0;
    last = f.in_dim;
    for (int l = 0; l < f.n_hidden; ++l) {
        for (int j = 0; j < f.hidden[l]; ++j)
            for (int k = 0; k < last; ++k) map[(size_t)f.off_w[l] + (size_t)k * FNN_W + j] = q++;
        for (int j = 0; j < f.hidden[l]; ++j) map[(size_t)f.off_b[l] + j] = q++;
        last = f.hidden[l];
    }
    for (int j = 0; j < ei.A; ++j)
        for (int k = 0; k < last; ++k) map[(size_t)f.off_w[f.n_hidden] + (size_t)j * FNN_W + k] = q++;
    for (int j = 0; j < ei.A; ++j) map[(size_t)f.off_b[f.n_hidden] + j] = q++;
    if (int rc = upload_packed(h, who, map, params, need, &f.w)) return rc;
    h->fnn = f;
    h->pol_map = std::move(map);
    h->pol_n_params = need;
    return VS_OK;
}

int vs_set_policy_rnn(vs_handle h, const vs_rnn_desc* desc, const float* params, int64_t n_params) {
    if (!h) return VS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (int rc = drop_policy(h)) return rc;  // before any check: a refused call leaves no policy
    if (!desc) return VS_OK;
    const EnvInfo& ei = ENV_INFO[h->type];
    const char* who = "vs_set_policy_rnn";
    if (h->type == VS_ENV_BOB_D) return fail(h, VS_ERR_ARG, "vs_set_policy_rnn: the discrete-action family takes no network policy");
    if (h->d.pipe.act_on || h->d.pipe.obs_on) return fail(h, VS_ERR_STATE, "vs_set_policy_rnn: not available with a wrapper pipeline on the handle");
    if (!params || desc->cell < VS_RNN_TANH || desc->cell > VS_RNN_LSTM) return fail(h, VS_ERR_ARG, "vs_set_policy_rnn: unknown cell kind or no parameter vector");
    if (desc->n_layers < 1 || desc->n_layers > RNN_MAXL) return fail(h, VS_ERR_ARG, "vs_set_policy_rnn: 1 .. 2 recurrent layers");
    if (desc->hidden < 1 || desc->hidden > RNN_MAXW) return fail(h, VS_ERR_ARG, "vs_set_policy_rnn: 1 .. 64 hidden units");
    if (desc->out_nonlin < 0 || desc->out_nonlin > FNN_SIGMOID) return fail(h, VS_ERR_ARG, "vs_set_policy_rnn: unknown nonlinearity");
    Rnn f{};
    f.cell = desc->cell;
    f.n_layers = desc->n_layers;
    f.hidden = desc->hidden;
    f.hp = (f.hidden + 3) / 4 * 4;
    const int G = rnn_gates(f.cell), lstm = f.cell == VS_RNN_LSTM;
    f.hs = f.n_layers * f.hidden * (lstm ? 2 : 1);
    f.out_nonlin = desc->out_nonlin;
    if (int rc = policy_view(h, who, *desc, f)) return rc;  // (at most O <= MAXO = RNN_XP rows: they fit the padded input row)
    if (int rc = policy_noise(h, who, *desc, f)) return rc;
    const int64_t Hh = f.hidden;
    int64_t need = 0;
    int off = 0;
    for (int l = 0; l < f.n_layers; ++l) {
        const int64_t in = l == 0 ? f.n_vis : Hh;
        need += G * Hh * in + G * Hh * Hh + 2 * G * Hh;
        f.off[l] = off;
        f.blk[l] = ((l == 0 ? RNN_XP : f.hp) + f.hp) * G + (2 * G + 3) / 4 * 4;
        off += f.blk[l] * f.hidden;
    }
    need += (int64_t)ei.A * Hh + ei.A;
    f.off_o = off;
    off += ei.A * f.hp + 4;
    if (n_params != need) return fail(h, VS_ERR_ARG, "vs_set_policy_rnn: parameter count does not match the cell, layers and sizes");
    f.lds_rows = (f.n_layers * (lstm ? 2 : 1) + f.n_layers) * f.hp;
    // torch order -> per unit blocks, gate-interleaved rows (the kernel reads G consecutive floats per input); an index map
    // as in vs_set_policy_fnn
    std::vector<int> map((size_t)off, -1);
    int q = 0;
    for (int l = 0; l < f.n_layers; ++l) {
        const int in = l == 0 ? f.n_vis : f.hidden, inp = l == 0 ? RNN_XP : f.hp;
        auto unit = [&](int row) { return (size_t)f.off[l] + (size_t)(row % f.hidden) * f.blk[l]; };  // row = g H + j of torch
        for (int r = 0; r < G * f.hidden; ++r)  // weight_ih [G H][in]
            for (int k = 0; k < in; ++k) map[unit(r) + (size_t)k * G + r / f.hidden] = q++;
        for (int r = 0; r < G * f.hidden; ++r)  // weight_hh [G H][H]
            for (int k = 0; k < f.hidden; ++k) map[unit(r) + (size_t)(inp + k) * G + r / f.hidden] = q++;
        for (int r = 0; r < G * f.hidden; ++r) map[unit(r) + (size_t)(inp + f.hp) * G + r / f.hidden] = q++;      // bias_ih
        for (int r = 0; r < G * f.hidden; ++r) map[unit(r) + (size_t)(inp + f.hp) * G + G + r / f.hidden] = q++;  // bias_hh
    }
    for (int j = 0; j < ei.A; ++j)
        for (int k = 0; k < f.hidden; ++k) map[(size_t)f.off_o + (size_t)j * f.hp + k] = q++;
    for (int j = 0; j < ei.A; ++j) map[(size_t)f.off_o + (size_t)ei.A * f.hp + j] = q++;
    if (int rc = upload_packed(h, who, map, params, need, &f.w)) return rc;
    const size_t hb = (size_t)f.hs * h->d.ld * sizeof(float);
    hipError_t e = hipMalloc((void**)&f.hid, hb);
    if (e == hipSuccess) e = hipMemset(f.hid, 0, hb);
    if (e != hipSuccess) { (void)hipFree((void*)f.w); if (f.hid) (void)hipFree(f.hid); return fail(h, VS_ERR_HIP, who, "hidden state", e); }
    h->rnn = f;
    h->pol_map = std::move(map);
    h->pol_n_params = need;
    return VS_OK;
}

int vs_set_policy_linear(vs_handle h, const vs_lin_desc* desc, const float* params, int64_t n_params) {
    if (!h) return VS_ERR_ARG;
    const char* who = "vs_set_policy_linear";
    Lin f{};
    std::vector<int> map;
    int64_t need = 0;
    if (desc) {  // every check before anything is dropped: a refused call leaves the previous policy and population in place
        const EnvInfo& ei = ENV_INFO[h->type];
        if (h->type == VS_ENV_BOB_D) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: the discrete-action family takes no in-kernel policy");
        if (h->d.pipe.act_on || h->d.pipe.obs_on) return fail(h, VS_ERR_STATE, "vs_set_policy_linear: not available with a wrapper pipeline on the handle");
        if (!params || desc->n_terms < 1 || desc->n_terms > VS_LIN_MAX_TERMS) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: 1 .. 51 terms and a parameter vector");
        if (int rc = policy_view(h, who, *desc, f)) return rc;
        if (int rc = policy_noise(h, who, *desc, f)) return rc;
        // feature q of the stack -> slot of a packed weight row (see k_rollout_lin)
        std::vector<int> slot;
        for (int t = 0; t < desc->n_terms; ++t) {
            const vs_lin_term& tm = desc->terms[t];
            if (tm.kind < 0 || tm.kind > VS_FEAT_ATAN2) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: unknown feature kind");
            if (tm.kind <= VS_FEAT_CONST) {
                if (f.kinds & (1u << tm.kind)) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: an elementwise kind (or the constant) appears twice in the stack");
                f.kinds |= 1u << tm.kind;
                if (tm.kind == VS_FEAT_CONST) slot.push_back(LIN_CONST_SLOT);
                else for (int k = 0; k < f.n_vis; ++k) slot.push_back(tm.kind * MAXO + k);
                continue;
            }
            const bool at = tm.kind == VS_FEAT_ATAN2;
            if (at ? tm.n_idx != 2 : (tm.n_idx < 2 || tm.n_idx > 4)) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: MultFeat takes 2 .. 4 rows, ATan2Feat 2");
            if (f.n_x >= LIN_MAXX) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: more than 39 MultFeat / ATan2Feat terms");
            unsigned xt = at ? 0x80000000u : ((unsigned)(tm.n_idx - 2) << 12);
            for (int r = 0; r < tm.n_idx; ++r) {
                if (tm.idx[r] < 0 || tm.idx[r] >= f.n_vis) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: a feature index outside the visible observation rows");
                xt |= (unsigned)f.obs_idx[tm.idx[r]] << (3 * r);
            }
            slot.push_back(LIN_CONST_SLOT + 1 + f.n_x);
            f.xterm[f.n_x++] = xt;
        }
        const int F = (int)slot.size();
        if (F > VS_LIN_MAX_FEAT) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: more than 128 features");
        need = (int64_t)ei.A * F;
        if (n_params != need) return fail(h, VS_ERR_ARG, "vs_set_policy_linear: parameter count is not (action dimensions) x (features)");
        map.assign((size_t)ei.A * LIN_SLOTS, -1);
        for (int j = 0; j < ei.A; ++j)
            for (int q = 0; q < F; ++q) map[(size_t)j * LIN_SLOTS + slot[q]] = j * F + q;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (desc)
        if (int rc = upload_packed(h, who, map, params, need, &f.w)) return rc;
    if (int rc = drop_policy(h)) return rc;
    if (!desc) return VS_OK;
    h->lin = f;
    h->pol_map = std::move(map);
    h->pol_n_params = need;
    return VS_OK;
}

// the caller's table (host or device) in the kernel's layout: a new device buffer [rw][n_rec rounded up to 64]
static int relay_table(vs_handle h, const char* who, const float* src, int n_rec, int64_t rw, float** out) {
    const int nrl = (n_rec + 63) / 64 * 64;
    const int64_t total = rw * nrl;
    float *tmp = nullptr, *dst = nullptr;
    hipError_t e = hipSuccess;
    if (!is_device_ptr(src)) {
        const size_t bytes = (size_t)n_rec * (size_t)rw * sizeof(float);
        e = hipMalloc((void**)&tmp, bytes);
        if (e == hipSuccess) e = hipMemcpy(tmp, src, bytes, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&dst, (size_t)total * sizeof(float));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_relay_table, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, tmp ? tmp : src, n_rec, rw, dst, nrl);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (the staging copy goes, and the caller's table may change)
    if (tmp) (void)hipFree(tmp);
    if (e != hipSuccess) {
        if (dst) (void)hipFree(dst);
        return fail(h, VS_ERR_HIP, who, e);
    }
    *out = dst;
    return VS_OK;
}

int vs_set_policy_playback(vs_handle h, const float* actions, int n_rec, int t_len, const int32_t* rec_len, const int32_t* lane_rec) {
    if (!h) return VS_ERR_ARG;
    const EnvInfo& ei = ENV_INFO[h->type];
    int nrl = 0;
    if (actions) {  // every check before anything is dropped: a refused call leaves the previous policy (and target) in place
        if (h->type == VS_ENV_BOB_D) return fail(h, VS_ERR_ARG, "vs_set_policy_playback: the discrete-action family takes no in-kernel policy");
        if (h->d.pipe.act_on || h->d.pipe.obs_on) return fail(h, VS_ERR_STATE, "vs_set_policy_playback: not available with a wrapper pipeline on the handle");
        if (n_rec < 1 || t_len < 1) return fail(h, VS_ERR_ARG, "vs_set_policy_playback: n_rec >= 1 and t_len >= 1");
        nrl = (n_rec + 63) / 64 * 64;
        if (((int64_t)t_len + 1) * MAXO * nrl > (int64_t)INT_MAX) return fail(h, VS_ERR_ARG, "vs_set_policy_playback: the table is too large (2^31 floats)");
        if (rec_len)
            for (int r = 0; r < n_rec; ++r)
                if (rec_len[r] < 0 || rec_len[r] > t_len) return fail(h, VS_ERR_ARG, "vs_set_policy_playback: rec_len outside [0, t_len]");
        if (lane_rec)
            for (int i = 0; i < h->d.n; ++i)
                if (lane_rec[i] < 0 || lane_rec[i] >= n_rec) return fail(h, VS_ERR_ARG, "vs_set_policy_playback: lane_rec outside [0, n_rec)");
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (a launch in flight may still read the tables this replaces)
    Play p{};
    if (actions) {
        float* da = nullptr;
        int *dl = nullptr, *dm = nullptr;
        if (int rc = relay_table(h, "vs_set_policy_playback: table upload", actions, n_rec, (int64_t)t_len * ei.A, &da)) return rc;
        std::vector<int> lens((size_t)nrl, 0);
        for (int r = 0; r < n_rec; ++r) lens[r] = rec_len ? rec_len[r] : t_len;
        hipError_t e = hipMalloc((void**)&dl, (size_t)nrl * sizeof(int));
        if (e == hipSuccess) e = hipMemcpy(dl, lens.data(), (size_t)nrl * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess && lane_rec) {
            std::vector<int> map((size_t)h->d.ld, 0);  // (lanes beyond n_envs replay recording 0: every read stays in the table)
            for (int i = 0; i < h->d.n; ++i) map[i] = lane_rec[i];
            e = hipMalloc((void**)&dm, map.size() * sizeof(int));
            if (e == hipSuccess) e = hipMemcpy(dm, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            (void)hipFree(da);
            if (dl) (void)hipFree(dl);
            if (dm) (void)hipFree(dm);
            return fail(h, VS_ERR_HIP, "vs_set_policy_playback: upload", e);
        }
        p.act = da;
        p.rec_len = dl;
        p.lane_rec = dm;
        p.n_rec = n_rec;
        p.n_rec_ld = nrl;
        p.t_len = t_len;
    }
    if (int rc = drop_policy(h)) return rc;
    h->play = p;
    return VS_OK;
}

int vs_set_rollout_target(vs_handle h, const float* target_obs, int n_rec, int t_len, const float* weights) {
    if (!h) return VS_ERR_ARG;
    const EnvInfo& ei = ENV_INFO[h->type];
    HIPCHK(h, hipSetDevice(h->device));
    if (!target_obs) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return drop_target(h);
    }
    if (!h->play.act) return fail(h, VS_ERR_STATE, "vs_set_rollout_target: no playback policy set (vs_set_policy_playback)");
    if (n_rec != h->play.n_rec || t_len != h->play.t_len) return fail(h, VS_ERR_ARG, "vs_set_rollout_target: n_rec and t_len must equal the playback policy's");
    float w[MAXO];
    for (int q = 0; q < MAXO; ++q) {
        w[q] = q < ei.O ? (weights ? weights[q] : 1.f) : 0.f;
        if (!(w[q] >= 0.f)) return fail(h, VS_ERR_ARG, "vs_set_rollout_target: weights must be >= 0");
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (a launch in flight may still read the target this replaces)
    float *dt = nullptr, *dl = nullptr;
    if (int rc = relay_table(h, "vs_set_rollout_target: table upload", target_obs, n_rec, (int64_t)(t_len + 1) * ei.O, &dt)) return rc;
    hipError_t e = hipMalloc((void**)&dl, (size_t)h->d.ld * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(dl, 0, (size_t)h->d.ld * sizeof(float), h->stream);
    if (e != hipSuccess) {
        (void)hipFree(dt);
        if (dl) (void)hipFree(dl);
        return fail(h, VS_ERR_HIP, "vs_set_rollout_target: allocation", e);
    }
    // the old tables go, not drop_target(): a new target keeps the sensitivities on and zeroes their sums
    if (int rc = dfree(h, h->play.tgt, h->play.loss)) { (void)hipFree(dt); (void)hipFree(dl); return rc; }
    h->play.tgt = dt;
    h->play.loss = dl;
    for (int q = 0; q < MAXO; ++q) h->play.w[q] = w[q];
    if (h->sens.n) return zero_sens(h, nullptr);
    return VS_OK;
}

int vs_set_rollout_sens(vs_handle h, const int32_t* param_idx, int n_params) {
    if (!h) return VS_ERR_ARG;
    const EnvInfo& ei = ENV_INFO[h->type];
    if (n_params < 0 || n_params > VS_SENS_MAX_PARAMS) return fail(h, VS_ERR_ARG, "vs_set_rollout_sens: n_params outside 0 .. VS_SENS_MAX_PARAMS");
    if (n_params > 0) {  // every check before anything changes: a refused call leaves the handle as it was
        if (!param_idx) return fail(h, VS_ERR_ARG, "vs_set_rollout_sens: NULL param_idx");
        for (int j = 0; j < n_params; ++j) {
            if (param_idx[j] < 0 || param_idx[j] >= ei.P) return fail(h, VS_ERR_ARG, "vs_set_rollout_sens: a parameter index outside the family's list");
            for (int l = 0; l < j; ++l)
                if (param_idx[l] == param_idx[j]) return fail(h, VS_ERR_ARG, "vs_set_rollout_sens: a parameter index is repeated");
        }
        if (h->type == VS_ENV_BOB_D) return fail(h, VS_ERR_STATE, "vs_set_rollout_sens: the discrete-action family takes no playback policy");
        if (!h->play.act) return fail(h, VS_ERR_STATE, "vs_set_rollout_sens: no playback policy set (vs_set_policy_playback)");
        if (!h->play.tgt) return fail(h, VS_ERR_STATE, "vs_set_rollout_sens: no rollout target set (vs_set_rollout_target)");
        if (h->auto_reset) return fail(h, VS_ERR_STATE, "vs_set_rollout_sens: sensitivities run with auto-reset off");
        if (h->d.pipe.act_on || h->d.pipe.obs_on) return fail(h, VS_ERR_STATE, "vs_set_rollout_sens: not available with a wrapper pipeline on the handle");
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (a launch in flight may still use the buffers this replaces)
    if (n_params == 0) return drop_sens(h);
    Sens q{};
    q.n = n_params;
    q.np = n_params <= 2 ? n_params : 4;
    for (int j = 0; j < SENS_MAXP; ++j) q.idx[j] = j < n_params ? param_idx[j] : -1;
    const size_t ld = (size_t)h->d.ld;
    const size_t rows[3] = {(size_t)q.n, (size_t)(q.n * (q.n + 1) / 2), (size_t)((ei.S + ei.H) * q.np)};
    float* bufs[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int b = 0; b < 3 && e == hipSuccess; ++b) {
        e = hipMalloc((void**)&bufs[b], rows[b] * ld * sizeof(float));
        if (e == hipSuccess) e = hipMemsetAsync(bufs[b], 0, rows[b] * ld * sizeof(float), h->stream);
    }
    if (e != hipSuccess) {
        for (int b = 0; b < 3; ++b)
            if (bufs[b]) (void)hipFree(bufs[b]);
        return fail(h, VS_ERR_HIP, "vs_set_rollout_sens: allocation", e);
    }
    if (int rc = drop_sens(h)) {
        for (int b = 0; b < 3; ++b) (void)hipFree(bufs[b]);
        return rc;
    }
    q.grad = bufs[0];
    q.gn = bufs[1];
    q.sens = bufs[2];
    h->sens = q;
    return VS_OK;
}

int vs_set_policy_hidden_record(vs_handle h, int width) {
    if (!h || width < 0 || width > 2 * RNN_MAXL * RNN_MAXW * 4) return fail(h, VS_ERR_ARG, "vs_set_policy_hidden_record: bad width");
    if (width == h->hrec_width) return VS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->hrec_width = width;
    return alloc_hrec(h);
}

int vs_record_hidden(vs_handle h, const float* hidden, int64_t env_stride, int64_t dim_stride, int row) {
    if (!h || !hidden) return fail(h, VS_ERR_ARG, "vs_record_hidden: NULL argument");
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &st) != hipSuccess) (void)hipGetLastError();
    if (st == hipStreamCaptureStatusNone) {
        if (!is_device_ptr(hidden)) return fail(h, VS_ERR_ARG, "vs_record_hidden: the hidden state must be device memory");
        HIPCHK(h, hipSetDevice(h->device));
    }
    if (!h->d_hrec) return fail(h, VS_ERR_STATE, "vs_record_hidden: set the record capacity and vs_set_policy_hidden_record first");
    if (row >= h->traj_cap) return fail(h, VS_ERR_STATE, "vs_record_hidden: row exceeds vs_set_traj_capacity");
    hipLaunchKernelGGL(k_record_hidden, grid_for(h->d.ld), dim3(BLOCK), 0, h->stream, hidden, (long)env_stride, (long)dim_stride,
                       h->d_hrec, (const int*)h->d.rec_row, row, h->traj_cap, h->hrec_width, (size_t)h->d.ld, h->d.n);
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_set_policy_population(vs_handle h, const float* params, int64_t n_params, int n_sets, const int32_t* lane_set) {
    if (!h) return VS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (a launch in flight may still read the sets this replaces)
    if (!params) return drop_pop(h);
    if (h->play.act) return fail(h, VS_ERR_STATE, "vs_set_policy_population: a playback policy has no parameters to vary");
    if (!h->fnn.w && !h->rnn.w && !h->lin.w) return fail(h, VS_ERR_STATE, "vs_set_policy_population: no policy set (vs_set_policy_fnn / vs_set_policy_rnn / vs_set_policy_linear)");
    if (n_params != h->pol_n_params) return fail(h, VS_ERR_ARG, "vs_set_policy_population: parameter count does not match the policy's");
    if (n_sets < 1 || !lane_set) return fail(h, VS_ERR_ARG, "vs_set_policy_population: n_sets >= 1 and a lane table");
    // the set of every aligned group of 64 lanes (groups past n_envs: -1), and whether groups of 256 agree as well
    const int64_t n = h->d.n, ng = (int64_t)h->d.ld / 64;
    std::vector<int> wg((size_t)ng, -1);
    bool inert = false, g256 = true;
    for (int64_t g = 0; g * 64 < n; ++g) {
        const int s0 = lane_set[g * 64];
        for (int64_t i = g * 64; i < std::min(n, g * 64 + 64); ++i) {
            if (lane_set[i] < -1 || lane_set[i] >= n_sets) return fail(h, VS_ERR_ARG, "vs_set_policy_population: a set id outside -1 .. n_sets - 1");
            if (lane_set[i] != s0) return fail(h, VS_ERR_ARG, "vs_set_policy_population: every aligned group of 64 lanes must name one set (or be all -1)");
        }
        wg[(size_t)g] = s0;
        inert |= s0 < 0;
        if ((g & 3) != 0 && s0 != wg[(size_t)(g & ~3)]) g256 = false;  // (groups past n_envs run as invalid lanes of their 256)
    }
    if (int rc = drop_pop(h)) return rc;  // (a refused call above leaves the population as it was)
    // pack on the device: the policy packer's index map, one gather per set into rows of `stride` floats (a multiple of 64:
    // every set starts on its own 256-byte boundary)
    const int slots = (int)h->pol_map.size();
    const int64_t stride = ((int64_t)slots + 63) / 64 * 64;
    const float* src = params;
    float *tmp = nullptr, *dw = nullptr;
    int *dmap = nullptr, *dwg = nullptr;
    hipError_t e = hipSuccess;
    auto cleanup = [&]() {
        if (tmp) (void)hipFree(tmp);
        if (dmap) (void)hipFree(dmap);
    };
    if (!is_device_ptr(params)) {
        e = hipMalloc((void**)&tmp, (size_t)n_sets * n_params * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(tmp, params, (size_t)n_sets * n_params * sizeof(float), hipMemcpyHostToDevice);
        src = tmp;
    }
    if (e == hipSuccess) e = hipMalloc((void**)&dmap, (size_t)slots * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(dmap, h->pol_map.data(), (size_t)slots * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&dw, (size_t)n_sets * stride * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dwg, (size_t)ng * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(dwg, wg.data(), (size_t)ng * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_pack_population, dim3((unsigned)((stride + 255) / 256), (unsigned)std::min(n_sets, 65535)), dim3(256), 0,
                           h->stream, src, n_params, n_sets, (const int*)dmap, slots, dw, stride);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (the temporaries go below)
    cleanup();
    if (e != hipSuccess) {
        if (dw) (void)hipFree(dw);
        if (dwg) (void)hipFree(dwg);
        return fail(h, VS_ERR_HIP, "vs_set_policy_population: upload / pack", e);
    }
    h->pop = Pop{dw, dwg, stride};
    h->pp.wg_host = wg;  // (vs_pop_param_grad derives its partition from it)
    h->pop_sets = n_sets;
    h->pop_g256 = g256;
    h->pop_inert = inert;
    return VS_OK;
}

int vs_step_policy(vs_handle h, int k_steps, int record, uint64_t noise_seed) {
    if (!h || k_steps < 1) return fail(h, VS_ERR_ARG, "vs_step_policy: bad argument");
    if (h->pop.w) {  // the population kernels exist for sampling runs only: auto-reset off, records on
        if (h->auto_reset)
            return fail(h, VS_ERR_STATE, h->pop_inert ? "vs_step_policy: auto-reset with -1 lanes in the population table"
                                                      : "vs_step_policy: a population runs with auto-reset off");
        if (!record) return fail(h, VS_ERR_STATE, "vs_step_policy: a population runs with records on");
    }
    if (!h->fnn.w && !h->rnn.w && !h->lin.w && !h->play.act) return fail(h, VS_ERR_STATE, "vs_step_policy: no network set (vs_set_policy_fnn)");
    if (h->d.pipe.act_on || h->d.pipe.obs_on) return fail(h, VS_ERR_STATE, "vs_step_policy: not available with a wrapper pipeline on the handle");
    if (h->play.act) {
        if (h->play.tgt && h->auto_reset) return fail(h, VS_ERR_STATE, "vs_step_policy: a rollout target runs with auto-reset off");
        if (h->sens.n) {  // no records: the launch goes from here
            if (record) return fail(h, VS_ERR_STATE, "vs_step_policy: no records with sensitivities on (vs_set_rollout_sens)");
            if (h->auto_reset || !h->play.tgt) return fail(h, VS_ERR_STATE, "vs_step_policy: sensitivities need a rollout target and auto-reset off");
            HIPCHK(h, hipSetDevice(h->device));
            DISPATCH_ENV(h->type, Launch<E>::rollout_play_sens(h, k_steps));
            HIPCHK(h, hipGetLastError());
            return VS_OK;
        }
    }
    if (record && h->d.traj_t0 + k_steps > h->traj_cap) return fail(h, VS_ERR_STATE, "vs_step_policy: traj offset + k_steps exceeds vs_set_traj_capacity");
    if (h->rnn.w && record && h->hrec_width && h->hrec_width != h->rnn.hs)
        return fail(h, VS_ERR_STATE, "vs_step_policy: the hidden-state record width differs from the policy's hidden size");
    HIPCHK(h, hipSetDevice(h->device));
    const int rec = record ? h->record_mode : 0;
    if (h->play.act) {
        DISPATCH_ENV(h->type, Launch<E>::rollout_play(h, k_steps, rec));
    } else if (h->rnn.w) {
        h->rnn.hrec = h->d_hrec;
        DISPATCH_ENV(h->type, Launch<E>::rollout_rnn(h, k_steps, rec, noise_seed));
    } else if (h->lin.w) {
        DISPATCH_ENV(h->type, Launch<E>::rollout_lin(h, k_steps, rec, noise_seed));
    } else {
        int shape = fnn_shape(h);
        if (h->pop.w && shape != 0 && !h->pop_g256) {
            // the 256-env shapes take one set per workgroup of 256 lanes: a table that is uniform in groups of 64 only runs shape 0
            // when the choice is automatic, and is refused when shape 1 or 2 is pinned
            if (h->policy_shape > 0) return fail(h, VS_ERR_STATE, "vs_step_policy: the pinned 256-env shape needs a population table uniform in groups of 256 lanes");
            shape = 0;
        }
        DISPATCH_ENV(h->type, Launch<E>::rollout_fnn(h, k_steps, rec, noise_seed, shape));
    }
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_rollout_lengths(vs_handle h, int n_lanes, int t_steps, int64_t* lengths, uint8_t* done_last) {
    if (!h || n_lanes < 1 || n_lanes > h->d.n || t_steps < 1 || !lengths || !done_last)
        return fail(h, VS_ERR_ARG, "vs_rollout_lengths: bad argument");
    if (!h->d.traj_done || t_steps > h->traj_cap) return fail(h, VS_ERR_STATE, "vs_rollout_lengths: more steps than vs_set_traj_capacity holds");
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_rollout_lengths, dim3((unsigned)((n_lanes + 255) / 256)), dim3(256), 0, h->stream, (const uint32_t*)h->d.traj_done,
                       (size_t)h->d.ld, n_lanes, t_steps, (long long*)lengths, done_last, (const int*)h->pop.wg_set);
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_pack_traj(vs_handle h, int n_lanes, int t_steps, const int64_t* lengths, const int64_t* starts, float* rows) {
    if (!h || n_lanes < 1 || n_lanes > h->d.n || t_steps < 1 || !lengths || !starts || !rows)
        return fail(h, VS_ERR_ARG, "vs_pack_traj: bad argument");
    if (!h->d.traj_rec || t_steps > h->traj_cap) return fail(h, VS_ERR_STATE, "vs_pack_traj: more steps than vs_set_traj_capacity holds");
    if (((uintptr_t)rows & 3u) != 0) return fail(h, VS_ERR_ARG, "vs_pack_traj: the destination must be 4-byte aligned");
    HIPCHK(h, hipSetDevice(h->device));
    DISPATCH_ENV(h->type, Launch<E>::pack_traj(h, n_lanes, t_steps, (const long long*)lengths, (const long long*)starts, rows));
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

// What the three reverse-mode sweeps and vs_fnn_param_grad refuse alike, in one order and with the entry point's name in front;
// `policy` (may be NULL) names what the entry point needs of the handle's policy slot, or returns NULL; d_act / d_init are the two
// pointers the entry point cannot do without, `null_what` how it words their refusal.  Every refusal comes before the first device
// call and leaves the outputs untouched.
static int vjp_checks(vs_handle h, const char* who, int t_steps, const float* d_act, const float* d_init,
                      const char* (*policy)(vs_handle), const char* null_what = "NULL handle or output") {
    if (!h || !d_act || !d_init) return fail(h, VS_ERR_ARG, who, null_what);
    if (t_steps < 1) return fail(h, VS_ERR_ARG, who, "t_steps < 1");
    if (h->type == VS_ENV_BOB_D) return fail(h, VS_ERR_STATE, who, "the discrete-action family has no action gradient");
    if (const char* why = policy ? policy(h) : nullptr) return fail(h, VS_ERR_STATE, who, why);
    if (h->record_mode != 2) return fail(h, VS_ERR_STATE, who, "needs the records of record mode 2 (vs_set_record_mode)");
    if (h->auto_reset) return fail(h, VS_ERR_STATE, who, "switch auto-reset off (one rollout per lane, started at a reset)");
    if (h->d.pipe.act_on || h->d.pipe.obs_on) return fail(h, VS_ERR_STATE, who, "not available with a wrapper pipeline on the handle");
    if (h->d.traj_t0 != 0) return fail(h, VS_ERR_STATE, who, "set the trajectory offset back to 0 (the sweep reads rows 0 .. t_steps - 1)");
    if (t_steps > h->traj_cap || !h->d.traj_rec || !h->d.traj_done) return fail(h, VS_ERR_ARG, who, "t_steps exceeds vs_set_traj_capacity");
    return VS_OK;
}

// What the sweep entry points do once nothing is refused: the launch is the family's Launch<E>:: call, which may name `v`, the
// arguments every sweep takes (the entry point's own g_rew, g_obs, g_state_last, d_act and d_init).
#define VJP_LAUNCH(...)                                         \
    do {                                                        \
        HIPCHK(h, hipSetDevice(h->device));                     \
        const Vjp v{g_rew, g_obs, g_state_last, d_act, d_init}; \
        DISPATCH_ENV(h->type, __VA_ARGS__);                     \
        HIPCHK(h, hipGetLastError());                           \
        return VS_OK;                                           \
    } while (0)

int vs_rollout_vjp(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_state_last, float* d_act,
                   float* d_init) {
    if (int rc = vjp_checks(h, "vs_rollout_vjp", t_steps, d_act, d_init, nullptr)) return rc;
    VJP_LAUNCH(Launch<E>::rollout_vjp(h, v, t_steps));
}

int vs_rollout_vjp_params(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_state_last,
                          const int32_t* param_idx, int n_params, float* d_act, float* d_init, float* d_params) {
    const char* who = "vs_rollout_vjp_params";
    if (int rc = vjp_checks(h, who, t_steps, d_act, d_init, nullptr)) return rc;
    // the index checks of vs_set_rollout_sens
    if (!d_params) return fail(h, VS_ERR_ARG, who, "NULL d_params");
    if (n_params < 1 || n_params > VS_SENS_MAX_PARAMS) return fail(h, VS_ERR_ARG, who, "n_params outside 1 .. VS_SENS_MAX_PARAMS");
    if (!param_idx) return fail(h, VS_ERR_ARG, who, "NULL param_idx");
    const EnvInfo& ei = ENV_INFO[h->type];
    VjpDp q{};
    q.d_params = d_params;
    q.n = n_params;
    for (int j = 0; j < SENS_MAXP; ++j) q.idx[j] = -1;
    for (int j = 0; j < n_params; ++j) {
        if (param_idx[j] < 0 || param_idx[j] >= ei.P) return fail(h, VS_ERR_ARG, who, "a parameter index outside the family's list");
        for (int l = 0; l < j; ++l)
            if (param_idx[l] == param_idx[j]) return fail(h, VS_ERR_ARG, who, "a parameter index is repeated");
        q.idx[j] = param_idx[j];
    }
    VJP_LAUNCH(Launch<E>::rollout_vjp_dp(h, v, q, t_steps));
}

// what vs_rollout_vjp_policy and vs_lin_param_grad need of the policy slot
static const char* lin_sweep_policy(vs_handle h) {
    if (!h->lin.w) return "no linear policy on the handle (vs_set_policy_linear)";
    if (h->pop.w) return "not available with a policy population on the handle";
    return nullptr;
}

int vs_rollout_vjp_policy(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_act,
                          const float* g_state_last, float* d_act, float* d_init) {
    if (int rc = vjp_checks(h, "vs_rollout_vjp_policy", t_steps, d_act, d_init, lin_sweep_policy)) return rc;
    VJP_LAUNCH(Launch<E>::rollout_vjp_lin(h, v, g_act, t_steps));
}

// what vs_rollout_vjp_fnn and vs_fnn_param_grad need of the policy slot
static const char* fnn_sweep_policy(vs_handle h) {
    if (!h->fnn.w) return "no feed-forward network policy on the handle (vs_set_policy_fnn)";
    if (h->pop.w) return "not available with a policy population on the handle";
    if (h->fnn.n_hidden > 2) return "the sweep takes networks of one or two hidden layers";
    return nullptr;
}

int vs_rollout_vjp_fnn(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_act,
                       const float* g_state_last, float* d_act, float* d_init) {
    if (int rc = vjp_checks(h, "vs_rollout_vjp_fnn", t_steps, d_act, d_init, fnn_sweep_policy)) return rc;
    VJP_LAUNCH(Launch<E>::rollout_vjp_fnn(h, v, g_act, t_steps));
}

// what vs_rollout_vjp_rnn and vs_rnn_param_grad need of the policy slot
static const char* rnn_sweep_policy(vs_handle h) {
    if (!h->rnn.w) return "no recurrent policy on the handle (vs_set_policy_rnn)";
    if (h->pop.w) return "not available with a policy population on the handle";
    if (!h->d_hrec || h->hrec_width != h->rnn.hs)
        return "needs the hidden-state record plane at the policy's hidden size (vs_set_policy_hidden_record)";
    return nullptr;
}

int vs_rollout_vjp_rnn(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_act,
                       const float* g_state_last, const float* g_hid_last, float* d_act, float* d_init, float* d_hid, float* d_hid0) {
    if (int rc = vjp_checks(h, "vs_rollout_vjp_rnn", t_steps, d_act, d_init, rnn_sweep_policy)) return rc;
    VJP_LAUNCH(Launch<E>::rollout_vjp_rnn(h, v, g_act, g_hid_last, d_hid, d_hid0, t_steps));
}
// what vs_rollout_vjp_pop and vs_pop_param_grad need of the policy slot: a population of linear policies or of networks of one or two
// hidden layers (a recurrent policy's parameter pass has its own LDS layout; a playback policy has no parameters)
static const char* pop_sweep_policy(vs_handle h) {
    if (h->play.act) return "a playback policy has no parameters to vary";
    if (h->rnn.w) return "a population of recurrent policies has no sweep (linear and feed-forward policies only)";
    if (!h->lin.w && !h->fnn.w) return "no linear or feed-forward policy on the handle (vs_set_policy_linear / vs_set_policy_fnn)";
    if (!h->pop.w) return "no policy population on the handle (vs_set_policy_population)";
    if (h->fnn.w && h->fnn.n_hidden > 2) return "the sweep takes networks of one or two hidden layers";
    return nullptr;
}

int vs_rollout_vjp_pop(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_act,
                       const float* g_state_last, float* d_act, float* d_init) {
    if (int rc = vjp_checks(h, "vs_rollout_vjp_pop", t_steps, d_act, d_init, pop_sweep_policy)) return rc;
    VJP_LAUNCH(Launch<E>::rollout_vjp_pop(h, v, g_act, t_steps));
}
#undef VJP_LAUNCH

// ---- vs_fnn_param_grad / vs_rnn_param_grad / vs_lin_param_grad: one pass over the records a sweep read, a partial vector per workgroup, then one reduction
// What they refuse alike after vjp_checks, before the first device call (`what`: "network" or "policy"), and the records they read.
static int param_grad_checks(vs_handle h, const char* who, const char* what, int t_steps, int64_t n_params, FnnRows& rows) {
    if (n_params != h->pol_n_params)
        return fail(h, VS_ERR_ARG, who, (std::string("n_params is not the parameter count of the ") + what + " on the handle").c_str());
    if ((int64_t)(h->d.ld / 64) * t_steps > INT_MAX) return fail(h, VS_ERR_ARG, who, "more than 2^31 - 1 row tiles");
    const EnvInfo& ei = ENV_INFO[h->type];
    rows = FnnRows{h->d.traj_rec, h->d.traj_done, record_width(h->type, 2), ei.O, ei.A, h->d.n, h->d.ld};
    return VS_OK;
}

// workgroups of k_rnn_param_grad: a function of (ld, t_steps, device) only -- a workgroup per tile while there are fewer tiles than
// compute units (the LDS rows of a wide cell leave room for one workgroup on each), else one per compute unit, each a run of tiles
static int rnn_param_grad_wgs(const vs_env* h, int t_steps) {
    return (int)std::min<int64_t>((int64_t)(h->d.ld / 64) * t_steps, (int64_t)h->n_cu);
}

int vs_rnn_param_grad(vs_handle h, int t_steps, const float* abar, const float* d_hid, float* d_params, int64_t n_params,
                      int accumulate) {
    const char* who = "vs_rnn_param_grad";
    if (int rc = vjp_checks(h, who, t_steps, abar, d_params, rnn_sweep_policy, "NULL handle, abar or d_params")) return rc;
    if (!d_hid) return fail(h, VS_ERR_ARG, who, "NULL d_hid");
    FnnRows rows;
    if (int rc = param_grad_checks(h, who, "policy", t_steps, n_params, rows)) return rc;
    Rnn P = h->rnn;
    P.hrec = h->d_hrec;
    const int psize = (int)h->pol_map.size(), n_wg = rnn_param_grad_wgs(h, t_steps), G = rnn_gates(P.cell);
    if (psize != P.off_o + rows.A * P.hp + 4 || P.hp > RNN_MAXW || P.n_layers > RNN_MAXL)
        return fail(h, VS_ERR_STATE, who, "the packed layout is not vs_set_policy_rnn's");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = param_grad_workspace(h, who, psize, n_wg)) return rc;
    const size_t lds = rnng_lds_floats(G, P.n_layers, P.hp, rows.A) * sizeof(float);
    auto kern = G == 1 ? k_rnn_param_grad<1> : G == 3 ? k_rnn_param_grad<3> : k_rnn_param_grad<4>;
    // beyond the 64 KiB a kernel gets by default the limit is raised; refused, there is no launch
    if (lds > 64 * 1024)
        HIPCHK(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(64 * RNNG_WAVES), lds, h->stream, rows, abar, d_hid, P, t_steps, psize,
                       h->pg.part);
    launch_param_reduce(h, n_wg, psize, d_params, accumulate);
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

// workgroups of k_fnn_param_grad: a function of (ld, t_steps, device) only, so that the bits of a result do not depend on earlier
// calls -- a wave per tile while there are fewer tiles than wave slots, else two workgroups per compute unit, each wave a run of tiles
static int fnn_param_grad_wgs(const vs_env* h, int t_steps) {
    const int64_t tiles = (int64_t)(h->d.ld / 64) * t_steps;
    return (int)std::min<int64_t>((tiles + FNNG_WAVES - 1) / FNNG_WAVES, 2 * (int64_t)h->n_cu);
}

int vs_fnn_param_grad(vs_handle h, int t_steps, const float* abar, float* d_params, int64_t n_params, int accumulate) {
    const char* who = "vs_fnn_param_grad";
    if (int rc = vjp_checks(h, who, t_steps, abar, d_params, fnn_sweep_policy, "NULL handle, abar or d_params")) return rc;
    FnnRows rows;
    if (int rc = param_grad_checks(h, who, "network", t_steps, n_params, rows)) return rc;
    const Fnn& f = h->fnn;
    const int psize = (int)h->pol_map.size(), n_wg = fnn_param_grad_wgs(h, t_steps);
    if (psize != f.off_b[f.n_hidden] + 8 || psize > FNNG_PMAX) return fail(h, VS_ERR_STATE, who, "the packed layout is not vs_set_policy_fnn's");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = param_grad_workspace(h, who, psize, n_wg)) return rc;
    void (*kern)(FnnRows, const float*, Fnn, int, int, float*) = k_fnn_param_grad<1>;  // (the kernel without its population pack)
    if (f.n_hidden != 1) kern = k_fnn_param_grad<2>;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(64 * FNNG_WAVES), 0, h->stream, rows, abar, f, t_steps, psize, h->pg.part);
    launch_param_reduce(h, n_wg, psize, d_params, accumulate);
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

// workgroups of k_lin_param_grad, one wave each: a function of (ld, t_steps, device) only -- a wave per tile while there are fewer
// tiles than wave slots (the LDS rows of a wave leave room for four on a compute unit), else four per compute unit, each a run of tiles
static int lin_param_grad_wgs(const vs_env* h, int t_steps) {
    return (int)std::min<int64_t>((int64_t)(h->d.ld / 64) * t_steps, 4 * (int64_t)h->n_cu);
}

int vs_lin_param_grad(vs_handle h, int t_steps, const float* abar, float* d_params, int64_t n_params, int accumulate) {
    const char* who = "vs_lin_param_grad";
    if (int rc = vjp_checks(h, who, t_steps, abar, d_params, lin_sweep_policy, "NULL handle, abar or d_params")) return rc;
    FnnRows rows;
    if (int rc = param_grad_checks(h, who, "policy", t_steps, n_params, rows)) return rc;
    const int psize = (int)h->pol_map.size(), n_wg = lin_param_grad_wgs(h, t_steps);
    if (psize != rows.A * LIN_SLOTS || rows.A > MAXA) return fail(h, VS_ERR_STATE, who, "the packed layout is not vs_set_policy_linear's");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = param_grad_workspace(h, who, psize, n_wg)) return rc;
    void (*kern)(FnnRows, const float*, Lin, int, float*) = k_lin_param_grad<1>;  // (the kernel without its population pack)
    if (rows.A != 1) kern = k_lin_param_grad<2>;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(64), 0, h->stream, rows, abar, h->lin, t_steps, h->pg.part);
    launch_param_reduce(h, n_wg, psize, d_params, accumulate);
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

// ---- vs_pop_param_grad: the tile space partitioned by set of the population
// From the table's groups (set of every aligned group of 64 lanes, -1: inert or past n_envs):
//   ent   the groups that name a set, in stable order by (set, group): set s owns cnt_s consecutive entries
//   seg   per set {first workgroup, workgroups k_s}
//   wg    per workgroup {first entry of its set, cnt_s, rank among the set's workgroups, k_s}
// A set has cnt_s * t_steps tiles and `per_wg` tiles keep the waves of one workgroup busy, so it WANTS ceil(tiles_s / per_wg) workgroups.
// While all wants fit under `cap` (the grid cap of the single-policy pass) every set gets what it wants; beyond, set s gets
// floor(cap * tiles_s / tiles) of them, at least 1 and at most what it wants: shares in proportion to the sets' tiles, every named set
// served, at most n_sets workgroups above the cap.  A function of (table, t_steps, per_wg, cap) only.  tests/population_vjp_cases.py
// mirrors it line by line.
static int pop_partition(const std::vector<int>& groups, int n_sets, int t_steps, int per_wg, int64_t cap, std::vector<int>& ent,
                         std::vector<int>& wg, std::vector<int>& seg) {
    std::vector<int64_t> cnt((size_t)n_sets, 0), first((size_t)n_sets, 0);
    for (int s : groups)
        if (s >= 0) ++cnt[(size_t)s];
    int64_t n_ent = 0;
    for (int s = 0; s < n_sets; ++s) first[(size_t)s] = n_ent, n_ent += cnt[(size_t)s];
    ent.assign((size_t)n_ent, 0);
    std::vector<int64_t> at = first;
    for (size_t g = 0; g < groups.size(); ++g)
        if (groups[g] >= 0) ent[(size_t)at[(size_t)groups[g]]++] = (int)g;
    const int64_t tiles = n_ent * t_steps;
    int64_t want = 0;
    for (int s = 0; s < n_sets; ++s) want += (cnt[(size_t)s] * t_steps + per_wg - 1) / per_wg;
    seg.assign(2 * (size_t)n_sets, 0);
    wg.clear();
    int64_t n_wg = 0;
    for (int s = 0; s < n_sets; ++s) {
        const int64_t ts = cnt[(size_t)s] * t_steps, ws = (ts + per_wg - 1) / per_wg;
        int64_t k = ws;
        if (want > cap && ts > 0) k = std::min(ws, std::max<int64_t>(1, cap * ts / tiles));
        seg[2 * (size_t)s] = (int)n_wg, seg[2 * (size_t)s + 1] = (int)k;
        for (int64_t r = 0; r < k; ++r) {
            const int row[4] = {(int)first[(size_t)s], (int)cnt[(size_t)s], (int)r, (int)k};
            wg.insert(wg.end(), row, row + 4);
        }
        n_wg += k;
    }
    return (int)n_wg;
}

int vs_pop_partition(const int32_t* groups, int n_groups, int n_sets, int t_steps, int per_wg, int64_t cap, int32_t* seg, int32_t* wg,
                     int wg_cap, int32_t* ent) {
    if (!groups || n_groups < 1 || n_sets < 1 || t_steps < 1 || per_wg < 1 || cap < 1 || !seg) return VS_ERR_ARG;
    if ((int64_t)n_groups * t_steps > INT_MAX) return VS_ERR_ARG;
    for (int g = 0; g < n_groups; ++g)
        if (groups[g] < -1 || groups[g] >= n_sets) return VS_ERR_ARG;
    std::vector<int> e, w, s;
    const int n_wg = pop_partition(std::vector<int>(groups, groups + n_groups), n_sets, t_steps, per_wg, cap, e, w, s);
    std::copy(s.begin(), s.end(), seg);
    if (wg && n_wg <= wg_cap) std::copy(w.begin(), w.end(), wg);
    if (ent) std::copy(e.begin(), e.end(), ent);
    return n_wg;
}

// the partition for t_steps on the device: rebuilt when t_steps is not the last call's (a pure function: the bits of a result do not
// depend on what was built before)
static int pop_partition_upload(vs_handle h, const char* who, int t_steps, int per_wg, int64_t cap) {
    if (h->pp.t_steps == t_steps) return VS_OK;
    std::vector<int> ent, wg, seg;
    const int n_wg = pop_partition(h->pp.wg_host, h->pop_sets, t_steps, per_wg, cap, ent, wg, seg);
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (an earlier call may still read the tables this replaces)
    if (int rc = dfree(h, h->pp.ent, h->pp.wg, h->pp.seg)) return rc;
    h->pp.t_steps = h->pp.n_wg = 0;
    auto up = [&](int*& dst, const std::vector<int>& src) {
        hipError_t e = hipMalloc((void**)&dst, std::max<size_t>(src.size(), 4) * sizeof(int));
        if (e == hipSuccess && !src.empty()) e = hipMemcpy(dst, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = up(h->pp.ent, ent);
    if (e == hipSuccess) e = up(h->pp.wg, wg);
    if (e == hipSuccess) e = up(h->pp.seg, seg);
    if (e != hipSuccess) {
        (void)dfree(h, h->pp.ent, h->pp.wg, h->pp.seg);
        return fail(h, VS_ERR_HIP, who, "partition upload", e);
    }
    h->pp.t_steps = t_steps;
    h->pp.n_wg = n_wg;
    return VS_OK;
}

int vs_pop_param_grad(vs_handle h, int t_steps, const float* abar, float* d_params, int n_sets, int64_t n_params, int accumulate) {
    const char* who = "vs_pop_param_grad";
    if (int rc = vjp_checks(h, who, t_steps, abar, d_params, pop_sweep_policy, "NULL handle, abar or d_params")) return rc;
    if (n_sets != h->pop_sets) return fail(h, VS_ERR_ARG, who, "n_sets is not the population's");
    FnnRows rows;
    if (int rc = param_grad_checks(h, who, "policy", t_steps, n_params, rows)) return rc;
    const int psize = (int)h->pol_map.size();
    const Fnn& f = h->fnn;
    if (h->lin.w ? (psize != rows.A * LIN_SLOTS || rows.A > MAXA) : (psize != f.off_b[f.n_hidden] + 8 || psize > FNNG_PMAX))
        return fail(h, VS_ERR_STATE, who, "the packed layout is not the setter's");
    HIPCHK(h, hipSetDevice(h->device));
    // the grid caps of the single-policy passes: one wave per workgroup and four per compute unit (linear), four waves per workgroup
    // and two per compute unit (network)
    if (int rc = pop_partition_upload(h, who, t_steps, h->lin.w ? 1 : FNNG_WAVES, (h->lin.w ? 4 : 2) * (int64_t)h->n_cu)) return rc;
    const int n_wg = h->pp.n_wg;
    const PopSeg S{h->pop.w, h->pop.stride, h->pop.wg_set, h->pp.ent, (const int4*)h->pp.wg};
    if (n_wg > 0) {
        if (int rc = param_grad_workspace(h, who, psize, n_wg)) return rc;
        if (h->lin.w) {
            void (*kern)(FnnRows, const float*, Lin, int, float*, PopSeg) = k_lin_param_grad<1, PopSeg>;
            if (rows.A != 1) kern = k_lin_param_grad<2, PopSeg>;
            hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(64), 0, h->stream, rows, abar, h->lin, t_steps, h->pg.part, S);
        } else {
            void (*kern)(FnnRows, const float*, Fnn, int, int, float*, PopSeg) = k_fnn_param_grad<1, PopSeg>;
            if (f.n_hidden != 1) kern = k_fnn_param_grad<2, PopSeg>;
            hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(64 * FNNG_WAVES), 0, h->stream, rows, abar, f, t_steps, psize, h->pg.part, S);
        }
    } else if (int rc = param_grad_workspace(h, who, psize, 1)) {  // (no set is named: the reduction writes zeros; it needs the map)
        return rc;
    }
    hipLaunchKernelGGL((k_pop_param_reduce<4>), dim3((unsigned)((psize + BLOCK - 1) / BLOCK), (unsigned)std::min(n_sets, 65535)), dim3(BLOCK),
                       0, h->stream, (const float*)h->pg.part, (const int2*)h->pp.seg, n_sets, psize, (const int*)h->pg.map, d_params,
                       (long long)n_params, accumulate != 0 ? 1 : 0);
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

// what vs_noise_std_grad needs of the policy slot: a policy that adds NormalActNoiseExplStrat's noise, whatever its kind
static const char* noise_sweep_policy(vs_handle h) {
    if (!h->lin.w && !h->fnn.w && !h->rnn.w)
        return h->play.act ? "a playback policy adds no exploration noise" : "no linear, feed-forward or recurrent policy on the handle";
    if (h->pop.w) return "not available with a policy population on the handle";
    return nullptr;
}

// workgroups of k_noise_std_grad: a function of (ld, t_steps, device) only -- a wave per tile while there are fewer tiles than wave
// slots, else four workgroups of four waves per compute unit, each wave a contiguous run of tiles
static int noise_std_grad_wgs(const vs_env* h, int t_steps) {
    const int64_t tiles = (int64_t)(h->d.ld / 64) * t_steps;
    return (int)std::min<int64_t>((tiles + NSG_WAVES - 1) / NSG_WAVES, 4 * (int64_t)h->n_cu);
}

int vs_noise_std_grad(vs_handle h, int t_steps, uint64_t noise_seed, const float* abar, float* d_std, int accumulate, float* d_std_lane,
                      float* eps) {
    const char* who = "vs_noise_std_grad";
    // the eps-only call has neither abar nor a sum; every other call needs abar and d_std
    const bool eps_only = !abar && !d_std && !d_std_lane && eps;
    static const float some = 0.f;  // (stands in for the two pointers vjp_checks asks for, in the eps-only call)
    if (int rc = vjp_checks(h, who, t_steps, eps_only ? &some : abar, eps_only ? &some : d_std, noise_sweep_policy,
                            "NULL handle, abar or d_std (both may be NULL only when eps alone is asked for)"))
        return rc;
    if ((int64_t)(h->d.ld / 64) * t_steps > INT_MAX) return fail(h, VS_ERR_ARG, who, "more than 2^31 - 1 row tiles");
    const int A = ENV_INFO[h->type].A, n_wg = noise_std_grad_wgs(h, t_steps);
    if (A < 1 || A > 2) return fail(h, VS_ERR_STATE, who, "the noise of one Philox block serves one or two action rows");
    HIPCHK(h, hipSetDevice(h->device));
    if (d_std) {  // the workspace belongs to the policy slot (drop_policy frees it)
        if (!h->pg.nmap) {
            const int ident[2] = {0, 1};
            int* map = nullptr;
            HIPCHK(h, hipMalloc((void**)&map, sizeof(ident)));
            hipError_t e = hipMemcpy(map, ident, sizeof(ident), hipMemcpyHostToDevice);
            if (e != hipSuccess) { (void)hipFree(map); return fail(h, VS_ERR_HIP, who, "index map upload", e); }
            h->pg.nmap = map;
        }
        if (n_wg > h->pg.nwgs) {
            if (h->pg.npart) HIPCHK(h, hipStreamSynchronize(h->stream));  // (an earlier call may still read the smaller one)
            if (int rc = dfree(h, h->pg.npart)) return rc;
            h->pg.nwgs = 0;
            HIPCHK(h, hipMalloc((void**)&h->pg.npart, (size_t)n_wg * A * sizeof(float)));
            h->pg.nwgs = n_wg;
        }
    }
    const NoiseRows rows{h->d.traj_done, h->d.ep_idx, h->d.idx0, h->d.n, h->d.ld};
    auto kern = A == 1 ? k_noise_std_grad<1> : k_noise_std_grad<2>;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_wg), dim3(64 * NSG_WAVES), 0, h->stream, rows, noise_seed, abar, t_steps,
                       d_std ? h->pg.npart : (float*)nullptr, d_std_lane, eps);
    if (d_std)
        hipLaunchKernelGGL((k_fnn_param_reduce<4>), dim3(1), dim3(BLOCK), 0, h->stream, (const float*)h->pg.npart, n_wg, A,
                           (const int*)h->pg.nmap, d_std, accumulate != 0 ? 1 : 0);
    HIPCHK(h, hipGetLastError());
    return VS_OK;
}

int vs_returns_scan(int device_id, void* hip_stream, int64_t n, const int64_t* lengths, const int64_t* starts, const float* rew,
                    int64_t rew_stride, const float* values, int64_t values_stride, const uint8_t* done_last, float gamma, float lam,
                    int mode, float* out, float* out_first) {
    // every refusal comes before the first device call
    if (n <= 0 || n > INT32_MAX) return fail(nullptr, VS_ERR_ARG, "vs_returns_scan: n must be in 1 .. 2^31 - 1");
    if (!lengths || !starts || !rew || !out) return fail(nullptr, VS_ERR_ARG, "vs_returns_scan: lengths, starts, rew and out must not be NULL");
    if (mode != VS_RETURNS_RETURN && mode != VS_RETURNS_GAE) return fail(nullptr, VS_ERR_ARG, "vs_returns_scan: unknown mode");
    if (mode == VS_RETURNS_GAE && !values) return fail(nullptr, VS_ERR_ARG, "vs_returns_scan: VS_RETURNS_GAE needs values");
    if (rew_stride < 1 || (values && values_stride < 1)) return fail(nullptr, VS_ERR_ARG, "vs_returns_scan: a row stride below 1");
    if (!(gamma >= 0.f && gamma <= 1.f)) return fail(nullptr, VS_ERR_ARG, "vs_returns_scan: gamma outside [0, 1]");
    if (!(lam >= 0.f && lam <= 1.f)) return fail(nullptr, VS_ERR_ARG, "vs_returns_scan: lam outside [0, 1]");
    HIPCHK(nullptr, hipSetDevice(device_id));
    int cus = 0;
    HIPCHK(nullptr, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id));
    // the number of rows is device data (starts[n - 1] + lengths[n - 1] + n): a grid that fills the chip walks the tiles
    const dim3 tiles((unsigned)(cus > 0 ? cus * 8 : 2048)), blk(256);
    hipStream_t st = (hipStream_t)hip_stream;
    const int gae = mode == VS_RETURNS_GAE;
    const float c = gae ? (float)((double)gamma * (double)lam) : gamma;  // one rounding
    const long long *len = (const long long*)lengths, *sta = (const long long*)starts;
    hipLaunchKernelGGL(k_returns_scan, tiles, blk, 0, st, (int)n, len, sta, rew, (long long)rew_stride, values, (long long)values_stride,
                       done_last, gamma, c, gae, out);
    hipLaunchKernelGGL(k_returns_carry, dim3((unsigned)((n + 255) / 256)), blk, 0, st, (int)n, len, sta, c, out, out_first);
    hipLaunchKernelGGL(k_returns_apply, tiles, blk, 0, st, (int)n, len, sta, c, out);
    HIPCHK(nullptr, hipGetLastError());
    return VS_OK;
}

int vs_set_episode_log(vs_handle h, int on) {
    if (!h) return VS_ERR_ARG;
    h->d.log_episodes = on != 0;
    return VS_OK;
}

int vs_mixed_create(const vs_handle* handles, int n, vs_mixed_handle* out) {
    if (!handles || !out || n < 1 || n > MAX_SEG) return fail(nullptr, VS_ERR_ARG, "vs_mixed_create: need 1..5 handles");
    *out = nullptr;
    for (int q = 0; q < n; ++q) {
        if (!handles[q]) return fail(nullptr, VS_ERR_ARG, "vs_mixed_create: NULL handle");
        if (handles[q]->device != handles[0]->device) return fail(nullptr, VS_ERR_ARG, "vs_mixed_create: handles on different devices");
        if (handles[q]->auto_reset != handles[0]->auto_reset) return fail(nullptr, VS_ERR_ARG, "vs_mixed_create: handles differ in auto-reset");
        for (int p = 0; p < q; ++p)  // a segment is a handle's own buffers: two segments on one handle would race on them
            if (handles[p] == handles[q]) return fail(nullptr, VS_ERR_ARG, "vs_mixed_create: the same handle twice");
    }
    vs_mixed* m = new (std::nothrow) vs_mixed();
    if (!m) return fail(nullptr, VS_ERR_HIP, "vs_mixed_create: out of host memory");
    m->n = n;
    for (int q = 0; q < n; ++q) {
        m->sub[q] = handles[q];
        handles[q]->stream = handles[0]->stream;  // one launch, one stream
    }
    if (hipSetDevice(handles[0]->device) != hipSuccess || hipMalloc((void**)&m->dev, sizeof(Segs)) != hipSuccess) {
        delete m;
        return fail(nullptr, VS_ERR_HIP, "vs_mixed_create: hipMalloc failed");
    }
    *out = m;
    return VS_OK;
}

int vs_mixed_destroy(vs_mixed_handle m) {
    if (!m) return VS_OK;
    if (m->dev) (void)hipFree(m->dev);
    delete m;
    return VS_OK;
}

const char* vs_mixed_last_error(vs_mixed_handle m) { return m ? m->err.c_str() : ""; }

int vs_mixed_step_random(vs_mixed_handle m, uint64_t seed, int k_steps, int record) {
    if (!m) return VS_ERR_ARG;
    if (k_steps < 1) { m->err = "vs_mixed_step_random: k_steps must be >= 1"; return VS_ERR_ARG; }
    int rc = mixed_check(m, "vs_mixed_step_random", true, k_steps, record);
    if (rc) return rc;
    if (hipSetDevice(m->sub[0]->device) != hipSuccess) return VS_ERR_HIP;
    rc = mixed_upload(m, nullptr, nullptr, nullptr, k_steps);
    if (rc) return rc;
    launch_rollout_mixed((const Segs*)m->dev, m->total_blocks, m->sub[0]->stream, m->sub[0]->auto_reset,
                         record ? m->sub[0]->record_mode : 0, k_steps, seed, mixed_redraws(m));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { m->err = hipGetErrorString(e); return VS_ERR_HIP; }
    return VS_OK;
}

int vs_mixed_step(vs_mixed_handle m, const float* const* actions, const int64_t* env_strides, const int64_t* dim_strides) {
    if (!m) return VS_ERR_ARG;
    if (!actions || !env_strides || !dim_strides) { m->err = "vs_mixed_step: NULL argument"; return VS_ERR_ARG; }
    for (int q = 0; q < m->n; ++q)
        if (!actions[q] || !is_device_ptr(actions[q])) { m->err = "vs_mixed_step: actions must be device memory"; return VS_ERR_ARG; }
    int rc = mixed_check(m, "vs_mixed_step", false, 0, 0);
    if (rc) return rc;
    if (hipSetDevice(m->sub[0]->device) != hipSuccess) return VS_ERR_HIP;
    rc = mixed_upload(m, actions, env_strides, dim_strides, 0);
    if (rc) return rc;
    launch_step_mixed((const Segs*)m->dev, m->total_blocks, m->sub[0]->stream, m->sub[0]->auto_reset, mixed_redraws(m));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { m->err = hipGetErrorString(e); return VS_ERR_HIP; }
    return VS_OK;
}

int vs_mixed_time_random(vs_mixed_handle m, uint64_t seed, int k_steps, int record, int iters, float* avg_ms) {
    if (!m || !avg_ms || iters < 1) return VS_ERR_ARG;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return VS_ERR_HIP;
    int rc = vs_mixed_step_random(m, seed, k_steps, record);
    hipStream_t st = m->sub[0]->stream;
    if (rc == VS_OK) {
        (void)hipEventRecord(e0, st);
        for (int it = 0; it < iters && rc == VS_OK; ++it) rc = vs_mixed_step_random(m, seed, k_steps, record);
        (void)hipEventRecord(e1, st);
        float ms = 0.f;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = VS_ERR_HIP;
        *avg_ms = ms / (float)iters;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

int vs_clear_episodes(vs_handle h) {
    if (!h) return VS_ERR_ARG;
    HIPCHK(h, hipMemsetAsync(h->d.ep_count, 0, sizeof(unsigned), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d.es_count, 0, (size_t)h->d.ld * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d.es_retsum, 0, (size_t)h->d.ld * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d.es_lensum, 0, (size_t)h->d.ld * 4, h->stream));
    return VS_OK;
}

static bool buf_info(vs_handle h, int which, void** p, size_t* bytes) {
    const EnvInfo& ei = ENV_INFO[h->type];
    Dev& d = h->d;
    size_t ld = d.ld;
    switch (which) {
        case VS_STATE: *p = d.state; *bytes = ei.S * ld * 4; return true;
        case VS_OBS: *p = d.obs; *bytes = ei.O * ld * 4; return true;
        case VS_REW: *p = d.rew; *bytes = ld * 4; return true;
        case VS_DONE: *p = d.done; *bytes = ld; return true;
        case VS_HIDDEN: *p = d.hidden; *bytes = (size_t)ei.H * ld * 4; return true;
        case VS_STEPCOUNT: *p = d.step; *bytes = ld * 4; return true;
        case VS_ERRFLAG: *p = d.err; *bytes = ld; return true;
        case VS_RETURNS: *p = d.ret; *bytes = ld * 4; return true;
        case VS_PARAMS: *p = d.params; *bytes = ei.P * ld * 4; return true;
        case VS_CONSTS: *p = d.consts; *bytes = ei.K * ld * 4; return true;
        case VS_EP_RETURNS: *p = d.ep_ret; *bytes = (size_t)d.ep_cap * 4; return true;
        case VS_EP_LENGTHS: *p = d.ep_len; *bytes = (size_t)d.ep_cap * 4; return true;
        case VS_EP_ENVIDX: *p = d.ep_env; *bytes = (size_t)d.ep_cap * 4; return true;
        case VS_EP_COUNT: *p = d.ep_count; *bytes = 4; return true;
        case VS_TRAJ_REC: *p = d.traj_rec; *bytes = (size_t)h->traj_cap * record_width(h->type, h->record_mode) * ld * 4; return true;
        case VS_TRAJ_DONE: *p = d.traj_done; *bytes = (size_t)((h->traj_cap + 31) / 32) * ld * 4; return true;
        case VS_FAILED: *p = d.failed; *bytes = ld; return true;
        case VS_EPSTAT_COUNT: *p = d.es_count; *bytes = ld * 4; return true;
        case VS_EPSTAT_RETSUM: *p = d.es_retsum; *bytes = ld * 4; return true;
        case VS_EPSTAT_LENSUM: *p = d.es_lensum; *bytes = ld * 4; return true;
        case VS_JAC_STATE: *p = d.jac_s; *bytes = d.jac_s ? (size_t)ei.S * (ei.S + ei.A) * ld * 4 : 0; return true;
        case VS_JAC_REW: *p = d.jac_r; *bytes = d.jac_r ? (size_t)(ei.S + ei.A) * ld * 4 : 0; return true;
        case VS_JAC_OBS: *p = d.jac_o; *bytes = d.jac_o ? (size_t)ei.O * (ei.S + ei.A) * ld * 4 : 0; return true;
        case VS_POLICY_HIDDEN: *p = h->rnn.hid; *bytes = h->rnn.hid ? (size_t)h->rnn.hs * ld * 4 : 0; return true;
        case VS_ROLLOUT_LOSS: *p = h->play.loss; *bytes = h->play.loss ? ld * 4 : 0; return true;
        case VS_ROLLOUT_GRAD: *p = h->sens.grad; *bytes = h->sens.n ? (size_t)h->sens.n * ld * 4 : 0; return true;
        case VS_ROLLOUT_GN: *p = h->sens.gn; *bytes = h->sens.n ? (size_t)(h->sens.n * (h->sens.n + 1) / 2) * ld * 4 : 0; return true;
        case VS_ROLLOUT_SENS: *p = h->sens.sens; *bytes = h->sens.n ? (size_t)(ei.S + ei.H) * h->sens.np * ld * 4 : 0; return true;
        case VS_POLICY_HIDDEN_REC: *p = h->d_hrec; *bytes = h->d_hrec ? (size_t)h->traj_cap * h->hrec_width * ld * 4 : 0; return true;
#ifdef VS_WS_STAMP
        case 99: *p = d.dbg; *bytes = (size_t)(ld / 64) * 12 * 8; return true;
#endif

        default: return false;
    }
}

void* vs_get(vs_handle h, int which) {
    if (!h) return nullptr;
    void* p; size_t b;
    if (!buf_info(h, which, &p, &b)) { fail(h, VS_ERR_ARG, "vs_get: unknown buffer"); return nullptr; }
    return p;
}

int vs_copy_to_host(vs_handle h, int which, void* dst) {
    if (!h || !dst) return fail(h, VS_ERR_ARG, "vs_copy_to_host: NULL argument");
    void* p; size_t b;
    if (!buf_info(h, which, &p, &b)) return fail(h, VS_ERR_ARG, "vs_copy_to_host: unknown buffer");
    if (b == 0) return VS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(dst, p, b, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VS_OK;
}

int vs_copy_from_host(vs_handle h, int which, const void* src) {
    if (!h || !src) return fail(h, VS_ERR_ARG, "vs_copy_from_host: NULL argument");
    if (which != VS_STATE && which != VS_HIDDEN && which != VS_STEPCOUNT && which != VS_POLICY_HIDDEN)
        return fail(h, VS_ERR_ARG, "vs_copy_from_host: only VS_STATE / VS_HIDDEN / VS_STEPCOUNT / VS_POLICY_HIDDEN are assignable");
    void* p; size_t b;
    buf_info(h, which, &p, &b);
    if (b == 0) return VS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(p, src, b, hipMemcpyHostToDevice, h->stream));
    if (which == VS_STATE) {
        DISPATCH_ENV(h->type, Launch<E>::observe(h));
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VS_OK;
}

int64_t vs_error_count(vs_handle h) {
    if (!h) return -1;
    if (hipSetDevice(h->device) != hipSuccess) return -1;
    if (hipMemsetAsync(h->d_counter, 0, 8, h->stream) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_count_err, grid_for(h->d.ld), dim3(BLOCK), 0, h->stream, h->d.err, h->d.n, h->d_counter);
    unsigned long long v = 0;
    if (hipMemcpyAsync(&v, h->d_counter, 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    return (int64_t)v;
}

int vs_time_step_kernel(vs_handle h, int mode, const float* actions, int64_t env_stride, int64_t dim_stride,
                        int k_steps, int record, int iters, float* avg_ms) {
    if (!h || !avg_ms || iters < 1) return fail(h, VS_ERR_ARG, "vs_time_step_kernel: bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    int rc = VS_OK;
    // recording launches rotate through the record buffer (as many k_steps-row slots as its capacity holds), so that a
    // capacity of several times the 256 MiB Infinity Cache makes the record stream a real HBM stream
    const int t0_saved = h->d.traj_t0;
    const int slots = (mode == 1 && record && k_steps > 0) ? (h->traj_cap / k_steps > 0 ? h->traj_cap / k_steps : 1) : 1;
    auto one = [&](int it) {
        if (mode == 0) return vs_step(h, actions, env_stride, dim_stride);
        if (record) h->d.traj_t0 = (it % slots) * k_steps;
        return vs_step_random(h, 1234, k_steps, record);
    };
    // events on the stream the kernels are launched on; one warm launch first
    rc = one(0);
    if (rc == VS_OK) {
        (void)hipEventRecord(e0, h->stream);
        for (int it = 0; it < iters && rc == VS_OK; ++it) rc = one(it + 1);
        (void)hipEventRecord(e1, h->stream);
        hipError_t e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) rc = fail(h, VS_ERR_HIP, "vs_time_step_kernel: event timing", e);
        *avg_ms = ms / (float)iters;
    }
    h->d.traj_t0 = t0_saved;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

int vs_timer_start(vs_handle h) {
    if (!h) return VS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->ev0) {
        HIPCHK(h, hipEventCreate(&h->ev0));
        HIPCHK(h, hipEventCreate(&h->ev1));
    }
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    return VS_OK;
}

int vs_timer_stop(vs_handle h, float* ms) {
    if (!h || !ms) return fail(h, VS_ERR_ARG, "vs_timer_stop: NULL argument");
    if (!h->ev0) return fail(h, VS_ERR_STATE, "vs_timer_stop: vs_timer_start has not been called");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return VS_OK;
}

// mode 0: copy (read + write of `bytes`), mode 1: pure write stream
static int mem_probe(int device_id, int64_t bytes, int iters, float* gbps, int mode) {
    if (!gbps || bytes < (1 << 20) || iters < 1) return VS_ERR_ARG;
    if (hipSetDevice(device_id) != hipSuccess) return VS_ERR_HIP;
    void *a = nullptr, *b = nullptr;
    const size_t n4 = (size_t)bytes / 16;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return VS_ERR_HIP;
    if (hipMalloc(&a, n4 * 16) != hipSuccess) { (void)hipStreamDestroy(st); return VS_ERR_HIP; }
    if (mode == 0 && hipMalloc(&b, n4 * 16) != hipSuccess) { (void)hipFree(a); (void)hipStreamDestroy(st); return VS_ERR_HIP; }
    (void)hipMemsetAsync(a, 1, n4 * 16, st);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    const dim3 g((unsigned)((n4 + 256 * PROBE_V - 1) / (256 * PROBE_V))), blk(256);
    auto one = [&](int i) {
        if (mode == 0) hipLaunchKernelGGL(k_copy4, g, blk, 0, st, (const v4f*)a, (v4f*)b, n4);
        else hipLaunchKernelGGL(k_fill4, g, blk, 0, st, (v4f*)a, n4, (float)i);
    };
    one(0);
    (void)hipEventRecord(e0, st);
    for (int i = 0; i < iters; ++i) one(i + 1);
    (void)hipEventRecord(e1, st);
    hipError_t e = hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(a);
    if (b) (void)hipFree(b);
    (void)hipStreamDestroy(st);
    if (e != hipSuccess || ms <= 0.f) return VS_ERR_HIP;
    *gbps = (float)((mode == 0 ? 2.0 : 1.0) * (double)(n4 * 16) * iters / (ms * 1e-3) / 1e9);
    return VS_OK;
}

int vs_membw_probe(int device_id, int64_t bytes, int iters, float* gbps) { return mem_probe(device_id, bytes, iters, gbps, 0); }

int vs_memwrite_probe(int device_id, int64_t bytes, int iters, float* gbps) { return mem_probe(device_id, bytes, iters, gbps, 1); }

}  // extern "C"
