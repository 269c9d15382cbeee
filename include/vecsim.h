/*
 * vecsim.h -- C-ABI of libvecsim: an MI355X (gfx950) native, batched, device-resident stepper for Pyrado's
 * pure-Python simulated robots (SimPyEnv subclasses).
 *
 * The reference (swami1995/SimuRLacra, Pyrado) has no FFI for this path: the boundary is the Python duck type
 * Env/SimEnv consumed by rollout(), the env wrappers and the samplers.  Each entry point below is the batched
 * (N environments, one per wavefront lane) replacement of one reference method; the host-side mirror of the Python
 * surface lives in simurlacra_amd/ and calls these through ctypes (see INTEGRATION.md for the stub).
 * `P/` = Pyrado/pyrado/ in the reference tree.
 *
 * Conventions
 *   - every function returns an int status: 0 = VS_OK, < 0 = error (vs_last_error() gives the text); nothing throws;
 *   - the library owns all device buffers; callers get raw device pointers (vs_get) and never free them;
 *   - one handle <-> one HIP device + one stream; a handle is not re-entrant, independent handles are thread-safe;
 *   - all per-env arrays are fp32 struct-of-arrays [dim][ld] with row pitch ld = vs_ld() >= n_envs (rows 256-B
 *     aligned); done/err flags are uint8 [ld], step counters int32 [ld];
 *   - pointers passed IN (params, init states, actions, masks) may be host or device memory (detected with
 *     hipPointerGetAttributes) unless stated otherwise; SoA inputs use row pitch n_envs when they come from the
 *     host and an explicit pitch argument when they are device pointers.
 */
#ifndef VECSIM_H
#define VECSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_OK 0
#define VS_ERR_ARG (-1)     /* bad argument (shape, enum, null) -- pyrado.ShapeErr / ValueErr / TypeErr on the host side */
#define VS_ERR_HIP (-2)     /* a HIP runtime call failed (no device, OOM, launch error) */
#define VS_ERR_STATE (-3)   /* call order / handle state */
#define VS_ERR_NAN (-4)     /* NaN seen in an action or a state: BoxSpace.contains raises ValueErr, P/spaces/box.py:142-146 */

/* environment families (the `name` attribute of the reference classes) */
enum vs_env_type {
    VS_ENV_OMO = 0,    /* "omo"    OneMassOscillatorSim  P/environments/pysim/one_mass_oscillator.py:49-121 */
    VS_ENV_BOB = 1,    /* "bob"    BallOnBeamSim         P/environments/pysim/ball_on_beam.py:41-136 */
    VS_ENV_QQ_SU = 2,  /* "qq-su"  QQubeSwingUpSim       P/environments/pysim/quanser_qube.py:41-188 */
    VS_ENV_QCP_SU = 3, /* "qcp-su" QCartPoleSwingUpSim   P/environments/pysim/quanser_cartpole.py:45-230,507-587 */
    VS_ENV_QBB = 4,    /* "qbb"    QBallBalancerSim      P/environments/pysim/quanser_ball_balancer.py:49-337 */
    /* the remaining pysim families, sharing the kernels above */
    VS_ENV_QQ_ST = 5,  /* "qq-st"  QQubeStabSim          P/environments/pysim/quanser_qube.py:191-222 */
    VS_ENV_QCP_ST = 6, /* "qcp-st" QCartPoleStabSim      P/environments/pysim/quanser_cartpole.py:441-504 (flags default to long + simple) */
    VS_ENV_PEND = 7,   /* "pend"   PendulumSim           P/environments/pysim/pendulum.py:43-117 */
    VS_ENV_BOB_D = 8,  /* "bob-d"  BallOnBeamDiscSim     P/environments/pysim/ball_on_beam.py:139-161 */
    VS_ENV_COUNT = 9
};

/* buffers addressable through vs_get / vs_copy_to_host / vs_copy_from_host */
enum vs_buffer {
    VS_STATE = 0,      /* f32 [S][ld]  Env.state                                  P/environments/base.py:65 */
    VS_OBS = 1,        /* f32 [O][ld]  observe(state) after the last step/reset   P/environments/pysim/base.py:241 */
    VS_REW = 2,        /* f32 [ld]     reward of the last step (incl. final reward) base.py:220,237-239 */
    VS_DONE = 3,       /* u8  [ld]     done flag of the last step                 base.py:232-235 */
    VS_HIDDEN = 4,     /* f32 [H][ld]  qcp: _th_ddot, qbb: plate_angs             quanser_cartpole.py:74, quanser_ball_balancer.py:83 */
    VS_STEPCOUNT = 5,  /* i32 [ld]     Env.curr_step */
    VS_ERRFLAG = 6,    /* u8  [ld]     sticky: NaN seen in act/state (reference raises pyrado.ValueErr) */
    VS_RETURNS = 7,    /* f32 [ld]     undiscounted return of the running episode */
    VS_PARAMS = 8,     /* f32 [P][ld]  domain parameters, order = get_nominal_domain_param() */
    VS_CONSTS = 9,     /* f32 [K][ld]  derived constants (_calc_constants, bounds, c_max); layout in DESIGN.md */
    VS_EP_RETURNS = 10,/* f32 [ep_cap] episode log (vs_set_episode_log): completed-episode returns, append order (ring) */
    VS_EP_LENGTHS = 11,/* i32 [ep_cap] completed-episode lengths */
    VS_EP_ENVIDX = 12, /* i32 [ep_cap] env index of each completed episode */
    VS_EP_COUNT = 13,  /* u32 [1]      number of episodes appended since vs_clear_episodes */
    VS_TRAJ_REC = 14,  /* f32 [T][F * ld]: the records of a recording vs_step_random, one per env and step.
                        * record mode 1 (default), F = O + A + 1:
                        *   [obs BEFORE the step (O) | raw (unclipped) action of the policy (A) | reward]
                        * record mode 2 (vs_set_record_mode), F = O + A + 1 + S + A + H: everything rollout() keeps per step
                        * (P/sampling/rollout.py:237-258):
                        *   [... | state BEFORE the step (S) | applied action env.limit_act(act) (A) | hidden state BEFORE
                        *    the step (H; qcp: th_ddot)]
                        * Row t holds the F floats of every env split into planes of 4, 2 and 1 floats per env
                        * (F = 4 nq + 2 h2 + h1):
                        *   plane q < nq : f32 [ld][4] at float offset 4 ld q          <- record[4q .. 4q+3]
                        *   2-wide plane : f32 [ld][2] at 4 ld nq (if h2)              <- record[4nq], record[4nq+1]
                        *   1-wide plane : f32 [ld]    at (4 nq + 2 h2) ld (if h1)     <- record[F-1]
                        * so that a wavefront writes each plane with one dwordx4 / x2 / x1 store per lane, contiguously
                        * (vs_traj_layout reports nq, h2, h1). */
    VS_TRAJ_RESERVED_15 = 15,
    VS_TRAJ_RESERVED_16 = 16,
    VS_TRAJ_DONE = 17, /* u32 [ceil(T / 32)][ld]: done flag of recorded step t of env i = bit (t % 32) of word [t / 32][i].
                        * A lane keeps the running word in a register and a wave stores it once per 32 steps with one
                        * coalesced dword store (a byte per env and step was a 64-B partial-line store per wave and step) */
    VS_FAILED = 18,    /* u8  [ld]     Task.has_failed(state) of the last step   P/tasks/base.py:159-167 */
    VS_EPSTAT_COUNT = 19,  /* u32 [ld]  completed episodes per env since vs_clear_episodes */
    VS_EPSTAT_RETSUM = 20, /* f32 [ld]  sum of their undiscounted returns */
    VS_EPSTAT_LENSUM = 21, /* i32 [ld]  sum of their lengths */
    VS_JAC_STATE = 22,     /* f32 [S][S+A][ld]  d s'_j / d (s, a)_k of the last vs_step_jac */
    VS_JAC_REW = 23,       /* f32 [S+A][ld]     d r / d (s, a)_k */
    VS_JAC_OBS = 24,       /* f32 [O][S+A][ld]  d obs'_j / d (s, a)_k */
    VS_POLICY_HIDDEN = 25,     /* f32 [Hp][ld]  running hidden state of the recurrent policy of vs_set_policy_rnn, packed like
                                * Pyrado's: h of layer 0, 1 .. then (LSTM) c of layer 0, 1 .. (Hp = layers x hidden, x 2 for LSTM);
                                * zeroed by vs_set_policy_rnn, by vs_reset (the reset lanes) and per lane at every auto-reset */
    VS_POLICY_HIDDEN_REC = 26, /* f32 [T][W][ld] hidden-state record plane (vs_set_policy_hidden_record, W floats per env): row t =
                                * the policy's hidden state BEFORE recorded step t; same rows as VS_TRAJ_REC (capacity, offset) */
    VS_ROLLOUT_LOSS = 27,      /* f32 [ld]  per-lane discrepancy sum of vs_set_rollout_target (NULL / nothing copied without a target):
                                * zeroed by vs_set_rollout_target and by vs_reset (the reset lanes), accumulated by vs_step_policy */
    VS_ROLLOUT_GRAD = 28,      /* f32 [n_params][ld]  d VS_ROLLOUT_LOSS / d (chosen domain parameter j) of vs_set_rollout_sens (NULL /
                                * nothing copied while sensitivities are off) */
    VS_ROLLOUT_GN = 29,        /* f32 [n_params (n_params + 1) / 2][ld]  Gauss-Newton matrix sum w J^T J of the same sum: the upper
                                * triangle, row-major ((0,0) (0,1) .. (0,n-1) (1,1) ..) */
    VS_ROLLOUT_SENS = 30,      /* f32 [(S + H) * NP][ld]  the carried tangents d (state, hidden state) / d parameter, row
                                * (state row, then hidden row) * NP + tangent; NP = 1, 2 or 4 >= n_params */
    VS_BUFFER_COUNT = 31
};

/* vs_task_cfg.flags */
#define VS_FLAG_SIMPLE_DYNAMICS 1 /* qcp / qbb ctor arg simple_dynamics=True */
#define VS_FLAG_LONG_POLE 2       /* qcp ctor arg long=True (changes the nominal pole only) */
#define VS_FLAG_ACT_NORM 4        /* ActNormWrapper fused into the step: incoming actions live in [-1, 1] and are mapped to
                                     lb + (a + 1) (ub - lb) / 2 before anything else sees them
                                     (P/environment_wrappers/action_normalization.py:66-75) */
#define VS_FLAG_FREEZE_DONE 8     /* vs_set_freeze_done: vs_step leaves lanes alone whose done flag is set (rollout() stops at
                                     done, P/sampling/rollout.py:185); off by default -- env.step() after done keeps stepping */
#define VS_FLAG_LEAN_STEP 16      /* vs_set_lean_step: vs_step returns what SimPyEnv.step returns -- (obs, rew, done),
                                     P/environments/pysim/base.py:217-241 -- and keeps neither the running return VS_RETURNS nor
                                     the VS_FAILED byte */

/* Task / ctor configuration. Zero-initialise and set `use_defaults = 1` to get the reference defaults
 * (_create_task of each env).  Q and R are diagonal (all reference defaults are). */
typedef struct vs_task_cfg {
    int32_t use_defaults; /* 1: ignore state_des/q_diag/r_diag below */
    int32_t flags;        /* VS_FLAG_* */
    int32_t wild_init;    /* qcp: 0 = 'True' (default), 1 = 'False', 2 = anything else   quanser_cartpole.py:552-560 */
    int32_t reserved;
    float state_des[8];   /* task_args['state_des'] */
    float q_diag[8];      /* diag(task_args['Q']) */
    float r_diag[2];      /* diag(task_args['R']) */
    float init_state[8];  /* pend: the fixed initial state of its SingularStateSpace (ctor arg init_state) */
} vs_task_cfg;

/* One randomised domain parameter: DomainParam.sample = distr.sample -> clamp(clip_lo, clip_up)
 * (P/domain_randomization/domain_parameter.py:104-203) */
#define VS_DP_NORMAL 0  /* NormalDomainParam(mean, std)       spread = std */
#define VS_DP_UNIFORM 1 /* UniformDomainParam(mean, halfspan) spread = halfspan */
#define VS_DP_BERNOULLI 2 /* BernoulliDomainParam(val_0, val_1, prob_1) (domain_parameter.py:248-311):
                           * mean = val_0, spread = val_1, aux = prob_1 */
/* MultivariateNormalDomainParam (domain_parameter.py:206-245) of dimension 1 is VS_DP_NORMAL with spread = sqrt(cov);
 * higher dimensions put a vector under ONE parameter name, which no pysim env accepts */
typedef struct vs_dp_spec {
    int32_t param_index; /* row in VS_PARAMS */
    int32_t kind;        /* VS_DP_* */
    float mean;
    float spread;
    float clip_lo;       /* -INFINITY for none */
    float clip_up;       /* +INFINITY for none */
    float aux;           /* VS_DP_BERNOULLI: prob_1 */
    int32_t roundint;    /* DomainParam(roundint=True): round half to even after clipping (domain_parameter.py:127-129) */
} vs_dp_spec;

/* A feed-forward network policy for vs_step_policy: FNN(input, output, hidden_sizes, hidden_nonlin, output_nonlin)
 * of P/policies/feed_back/fnn.py:43-160 (dropout 0).  Hidden layers are at most 64 units wide. */
#define VS_NL_NONE 0
#define VS_NL_TANH 1
#define VS_NL_RELU 2
#define VS_NL_SIGMOID 3
#define VS_FNN_MAX_HIDDEN 4
#define VS_FNN_MAX_WIDTH 64
typedef struct vs_fnn_desc {
    int32_t n_hidden;          /* 1 .. VS_FNN_MAX_HIDDEN hidden layers */
    int32_t hidden[4];         /* their sizes, 1 .. VS_FNN_MAX_WIDTH each */
    int32_t hidden_nonlin[4];  /* VS_NL_* per hidden layer */
    int32_t output_nonlin;     /* VS_NL_* of the output layer */
    int32_t feat;              /* 0: the input is the visible observation; 1: the fork's FNNPolicy.forward featurisation
                                  [o_0, sin o_1, cos o_1, o_2 ..] (fnn.py:219-222; one input more than observation rows) */
    int32_t n_obs;             /* number of observation rows the policy sees; 0 = all of them, in order */
    int32_t obs_idx[8];        /* ... and which (ObsPartialWrapper, P/environment_wrappers/observation_partial.py:36-75) */
    float noise_std[2];        /* exploration: + std * N(0, 1) per action dimension (NormalActNoiseExplStrat); 0 = none */
} vs_fnn_desc;

/* A recurrent policy for vs_step_policy: torch.nn.RNN / GRU / LSTM (bias, batch_first = False, no dropout / projection, one
 * direction) and a Linear output layer -- RNNPolicy / GRUPolicy / LSTMPolicy of P/policies/recurrent/rnn.py. */
#define VS_RNN_TANH 0  /* nn.RNN(nonlinearity='tanh') */
#define VS_RNN_RELU 1  /* nn.RNN(nonlinearity='relu') */
#define VS_RNN_GRU 2   /* nn.GRU, gates r, z, n */
#define VS_RNN_LSTM 3  /* nn.LSTM, gates i, f, g, o */
#define VS_RNN_MAX_LAYERS 2
#define VS_RNN_MAX_HIDDEN 64
typedef struct vs_rnn_desc {
    int32_t cell;          /* VS_RNN_* */
    int32_t n_layers;      /* 1 .. VS_RNN_MAX_LAYERS */
    int32_t hidden;        /* units per layer, 1 .. VS_RNN_MAX_HIDDEN */
    int32_t out_nonlin;    /* VS_NL_* of the output layer */
    int32_t n_obs;         /* number of observation rows the policy sees; 0 = all of them, in order */
    int32_t obs_idx[8];    /* ... and which (as vs_fnn_desc) */
    float noise_std[2];    /* exploration: + std * N(0, 1) per action dimension (NormalActNoiseExplStrat); 0 = none */
} vs_rnn_desc;

/* A linear policy on a stack of feature functions for vs_step_policy: LinearPolicy(spec, feats=FeatureStack(...)) of
 * P/policies/feed_forward/linear.py over P/policies/features.py -- act = W phi(obs), W [A][F] without a bias.  The descriptor lists
 * the stack's terms in stack order.  An elementwise kind (VS_FEAT_IDENTITY .. VS_FEAT_SINCOS) maps every visible observation row
 * and so contributes n_obs features; VS_FEAT_CONST (the constant 1), VS_FEAT_MULT (MultFeat: the product of 2 .. 4 rows) and
 * VS_FEAT_ATAN2 (ATan2Feat: atan2(row idx[0], row idx[1])) contribute one each.  Their indices count the VISIBLE rows.
 * Limits: every elementwise kind and VS_FEAT_CONST at most once, at most VS_LIN_MAX_XTERMS MultFeat / ATan2Feat terms and at
 * most VS_LIN_MAX_FEAT features in all.  sin and cos come from the library's bounded-angle sincos: the fused linear policy is
 * valid for observations |obs| < ~1e3 (RBFFeat is not supported). */
#define VS_FEAT_IDENTITY 0 /* x */
#define VS_FEAT_SIGN 1     /* sign x */
#define VS_FEAT_ABS 2      /* |x| */
#define VS_FEAT_SQUARED 3  /* x^2 */
#define VS_FEAT_CUBIC 4    /* x^3 */
#define VS_FEAT_SIG 5      /* 1 / (1 + exp(-x)) */
#define VS_FEAT_BELL 6     /* exp(-x^2 / 2) */
#define VS_FEAT_SIN 7      /* sin x */
#define VS_FEAT_COS 8      /* cos x */
#define VS_FEAT_SINSIN 9   /* sin^2 x */
#define VS_FEAT_SINCOS 10  /* sin x cos x */
#define VS_FEAT_CONST 11   /* 1 (one feature) */
#define VS_FEAT_MULT 12    /* MultFeat(idcs): prod_r obs[idx[r]], n_idx = 2 .. 4 (one feature) */
#define VS_FEAT_ATAN2 13   /* ATan2Feat(idx_sin, idx_cos): atan2(obs[idx[0]], obs[idx[1]]), n_idx = 2 (one feature) */
#define VS_LIN_MAX_XTERMS 39
#define VS_LIN_MAX_TERMS 51 /* 12 + VS_LIN_MAX_XTERMS */
#define VS_LIN_MAX_FEAT 128
typedef struct vs_lin_term {
    int32_t kind;   /* VS_FEAT_* */
    int32_t n_idx;  /* VS_FEAT_MULT: 2 .. 4, VS_FEAT_ATAN2: 2, ignored otherwise */
    int32_t idx[4]; /* indices into the visible observation rows */
} vs_lin_term;
typedef struct vs_lin_desc {
    int32_t n_terms;                     /* 1 .. VS_LIN_MAX_TERMS */
    vs_lin_term terms[VS_LIN_MAX_TERMS]; /* the stack, in order */
    int32_t n_obs;                       /* number of observation rows the policy sees; 0 = all of them, in order */
    int32_t obs_idx[8];                  /* ... and which (as vs_fnn_desc) */
    float noise_std[2];                  /* exploration: + std * N(0, 1) per action dimension (NormalActNoiseExplStrat); 0 = none */
} vs_lin_desc;

typedef struct vs_env* vs_handle;

/* ---- static information (no GPU needed) ---- */

/* widths of an env family: state, action, observation, #domain params, hidden state, init-space element, #constants */
int vs_env_dims(int env_type, int* S, int* A, int* O, int* P, int* H, int* I, int* K);
/* the `name` class attribute ("qq-su", ...), NULL for a bad type */
const char* vs_env_name(int env_type);
/* i-th domain parameter name in get_nominal_domain_param() order, NULL when out of range */
const char* vs_param_name(int env_type, int i);
/* nominal domain parameters (get_nominal_domain_param; qcp honours VS_FLAG_LONG_POLE); out has P floats */
int vs_nominal_params(int env_type, int flags, float* out);
/* plane decomposition of a VS_TRAJ_REC row in record mode 1 or 2 (see vs_buffer): F = 4 * nq + 2 * h2 + h1 */
int vs_traj_layout(int env_type, int record_mode, int* F, int* nq, int* h2, int* h1);
/* library / ABI version */
int vs_version(void);

/* ---- lifetime ---- */

/* Replaces the env constructor (SimPyEnv.__init__, P/environments/pysim/base.py:46-80) for n_envs instances:
 * nominal domain params, derived constants, spaces and task.  max_steps <= 0 means pyrado.inf.  cfg may be NULL. */
int vs_create(int env_type, int64_t n_envs, double dt, int64_t max_steps, int device_id, const vs_task_cfg* cfg,
              vs_handle* out);
int vs_destroy(vs_handle h);
/* `env.max_steps = n` / `env.dt = h` (P/environments/base.py:73-104): plain attribute updates in the reference -- state,
 * step counters and running episodes are left alone; the new values apply from the next step.  max_steps <= 0: inf. */
int vs_set_max_steps(vs_handle h, int64_t max_steps);
int vs_set_dt(vs_handle h, double dt);
/* Streams.  A handle launches on its own stream, created as a blocking stream (hipStreamDefault): it is implicitly
 * ordered with the legacy default stream (torch's default "current stream"), so default-stream work may read the
 * handle's buffers (vs_get) after a launch without further synchronisation.  A caller that runs on another,
 * non-blocking stream (a torch side stream, a hipGraph capture stream) passes that hipStream_t here and the handle
 * launches on it; NULL restores the own stream.  For a loop that alternates the caller's default-stream work with vs_step,
 * pass hipStreamLegacy ((hipStream_t)1): on the very same stream there is no hand-over to pay for (the implicit
 * synchronisation between the legacy stream and a blocking stream costs ~25 us per step). */
int vs_set_stream(vs_handle h, void* hip_stream);
int vs_sync(vs_handle h);
int64_t vs_n_envs(vs_handle h);
int64_t vs_ld(vs_handle h);
const char* vs_last_error(vs_handle h); /* h may be NULL: last error of a failed vs_create on this thread */

/* ---- domain parameters: the `domain_param` setter (P/environments/pysim/base.py:112-124) ---- */

/* params_soa: f32 [P][pitch]; pitch = n_envs for host memory. mask (u8 [n_envs], may be NULL = all) selects the envs.
 * Recomputes _calc_constants, the spaces' bounds and the reward scale c_max for the selected envs. */
int vs_set_params(vs_handle h, const float* params_soa, int64_t pitch, const uint8_t* mask);
/* the same parameter vector (P floats, host) for every env; enables the broadcast-constant kernels */
int vs_set_params_uniform(vs_handle h, const float* params);
/* DomainRandomizer.randomize + get_params on device (P/domain_randomization/domain_randomizer.py:123-227):
 * Normal/Uniform draws (Philox4x32-10 keyed by seed), clipped; parameters without a spec keep their value. */
int vs_sample_params(vs_handle h, const vs_dp_spec* specs, int n_specs, uint64_t seed, const uint8_t* mask);
/* DomainRandWrapperBuffer (P/environment_wrappers/domain_randomization.py:151-261): a buffer of n_sets domain-parameter
 * sets, f32 [P][n_sets] (host memory); at each of its resets an env takes the next set (selection 0 = cyclic: lane i starts
 * at set (global index i) mod n_sets and advances by one per reset) or a random one (selection 1, Philox).
 * n_sets = 0 removes the buffer.  Mutually exclusive with vs_set_randomizer. */
int vs_set_param_buffer(vs_handle h, const float* params_soa, int n_sets, int selection);
/* toggle VS_FLAG_ACT_NORM after creation */
int vs_set_act_norm(vs_handle h, int on);
/* GaussianActNoiseWrapper (P/environment_wrappers/action_noise.py:38-79: act + randn * std + mean) and ActDelayWrapper
 * (P/environment_wrappers/action_delay.py:37-112: a queue of `delay` zero actions at reset, push the commanded action,
 * pop the oldest) fused into the step, applied after ActNormWrapper's de-normalisation and before the env's reward and
 * action clipping -- exactly where the wrapped env's step() would see them.
 *   delay              0 .. VS_MAX_ACT_DELAY time steps, the same for every env
 *   noise_mean/std     A floats each (host) or NULL for none
 *   noise_normed       the noise wrapper sits OUTSIDE ActNormWrapper: its draw is scaled by (ub - lb) / 2 of the env
 *   noise_after_delay  the noise wrapper sits INSIDE ActDelayWrapper (noise is added to the popped action)
 *   seed               Philox key of the noise; a draw is a pure function of (seed, global env index, episode, step)
 * vs_step_random draws the policy's action first and then runs it through this pipeline; the record holds the
 * policy's action.  delay = 0 and NULL noise removes the stage. */
#define VS_MAX_ACT_DELAY 64
int vs_set_act_pipeline(vs_handle h, int delay, const float* noise_mean, const float* noise_std, int noise_normed,
                        int noise_after_delay, uint64_t seed);
/* ObsNormWrapper (P/environment_wrappers/observation_normalization.py:41-126: (obs - lb) / (ub - lb) * 2 - 1) and
 * GaussianObsNoiseWrapper (P/environment_wrappers/observation_noise.py:38-73: obs + randn * std + mean), in any stacking
 * order, compose to   obs' = obs * scale + shift + noise_std * z,  z ~ N(0, 1) i.i.d.   (O floats each, host, NULL =
 * identity / none).  VS_OBS, the recorded observations and the observation vs_reset produces are the wrapped ones. */
int vs_set_obs_pipeline(vs_handle h, const float* scale, const float* shift, const float* noise_std, uint64_t seed);
/* DomainRandWrapperLive (P/environment_wrappers/domain_randomization.py:135-148): remember specs and redraw the
 * parameters of an env at each of its resets (vs_reset without explicit params, and auto-reset). n_specs = 0 disables. */
int vs_set_randomizer(vs_handle h, const vs_dp_spec* specs, int n_specs);

/* ---- reset: SimPyEnv.reset (P/environments/pysim/base.py:166-203) ---- */

/* init_state: NULL -> sample the env's init space on device (init_space.sample_uniform, P/spaces/box.py:169-178,
 * polar.py:108-113, compound.py:84-87); else f32 [I or S][pitch] (init_is_full_state selects which, base.py:184-193).
 * mask as above.  seed keys the Philox stream used for sampling (and for live domain randomisation). */
int vs_reset(vs_handle h, const float* init_state, int64_t pitch, int init_is_full_state, const uint8_t* mask,
             uint64_t seed);
/* Global index of lane 0 (default 0).  Every random stream of lane i is keyed by (first_global_index + i): a set of
 * envs gives the same trajectories whether it lives in one handle, is cut into batches, or is sharded over GPUs
 * (rank r of a node passes r * n_envs). */
int vs_set_index_offset(vs_handle h, uint32_t first_global_index);
/* when on, a lane whose episode ended is reset inside the same step kernel (fresh init state, redrawn params when a
 * randomizer is set); VS_OBS then holds the first observation of the new episode, VS_REW/VS_DONE the finished step */
int vs_set_auto_reset(vs_handle h, int on, uint64_t seed);

/* ---- step: SimPyEnv.step (P/environments/pysim/base.py:217-241), fused in one kernel ---- */

/* actions: device f32, element (env i, dim j) at actions[i * env_stride + j * dim_stride]
 * ([A][ld] SoA: env_stride 1, dim_stride ld;  [N][A] row-major policy output: env_stride A, dim_stride 1) */
int vs_step(vs_handle h, const float* actions, int64_t env_stride, int64_t dim_stride);
/* vs_step that also records the step (policy in the loop: rollout() with the caller's policy, rollout.py:185-258): the
 * observation the policy saw (VS_OBS as the previous step / the reset left it), its action, the reward and the done bit --
 * in record mode 2 also the state and hidden state before the step and env.limit_act(act) -- go into row `row` of the
 * VS_TRAJ_* buffers (same layout as the records of vs_step_random).  row < 0: the row comes from a device-side counter of
 * the handle (vs_set_record_row), which a one-thread kernel behind the step advances -- nothing host-side enters the
 * launch, so a captured hipGraph of (policy, vs_step_record) pairs replays correctly.  Rows beyond the capacity are skipped. */
int vs_step_record(vs_handle h, const float* actions, int64_t env_stride, int64_t dim_stride, int row);
int vs_set_record_row(vs_handle h, int row);
/* vs_step plus the step Jacobians d(s', r, obs') / d(s, a) (forward-mode differentiation of the same step code): what the
 * fork computes with torch autograd for its SAC-with-gradients (P/sampling/rollout.py:836-837 around
 * quanser_cartpole.py:233-431), for every family.  The raw action is the differentiation variable (a clipped or dead-zoned
 * action has zero gradient); hidden state is held constant; auto-reset must be off.  Values are bit-identical to vs_step. */
int vs_step_jac(vs_handle h, const float* actions, int64_t env_stride, int64_t dim_stride);
/* rollout() with DummyPolicy (P/sampling/rollout.py:185-239, P/policies/feed_forward/dummy.py:77-84):
 * k_steps env steps in ONE launch with on-device uniform actions in act_space, state kept in registers.
 * record != 0 streams obs/act/rew/done of every step into the VS_TRAJ_* buffers (k_steps <= vs_traj_capacity). */
int vs_step_random(vs_handle h, uint64_t seed, int k_steps, int record);
/* rollout() with a feed-forward network policy evaluated INSIDE the fused kernel (rollout.py:185-258 with act = policy(obs),
 * rollout.py:203-219): vs_set_policy_fnn hands over the network -- `params` is the policy's flat parameter vector in torch
 * order (per layer: weight [out][in] row-major, then bias [out]; hidden layers first, output layer last =
 * parameters_to_vector(FNN.parameters()), fnn.py:104-112), host or device memory, copied -- and vs_step_policy runs k_steps
 * env steps per launch: observation -> network -> (+ exploration noise) -> SimPyEnv.step -> record, exactly as
 * vs_step_random does with its uniform policy (same records, auto-reset and freeze semantics).  The noise stream is
 * Philox(noise_seed; global env index, episode index, step).  desc == NULL removes the network.
 * Not available with a wrapper pipeline on the handle or for the discrete-action family (VS_ERR_STATE / VS_ERR_ARG). */
int vs_set_policy_fnn(vs_handle h, const vs_fnn_desc* desc, const float* params, int64_t n_params);
int vs_step_policy(vs_handle h, int k_steps, int record, uint64_t noise_seed);
/* the shape vs_step_policy evaluates the network in: -1 automatic (default), 0 the network of 64 envs spread over the 8 waves
 * of a 64-env workgroup (vector ALU, lane = hidden unit), 1 the same in 256-env workgroups, 2 256-env workgroups with the
 * hidden layers on the matrix cores (v_mfma_f32_32x32x2_f32: fp32 in, fp32 out; one and two hidden layers -- deeper networks
 * run shape 0 whatever is asked).  No counterpart in the reference (which evaluates the torch module, P/sampling/rollout.py:203-219);
 * the shapes differ in the summation order of a layer only. */
int vs_set_policy_shape(vs_handle h, int shape);
/* vs_step_policy with a recurrent policy instead of a feed-forward one.  `params` is parameters_to_vector(policy.parameters())
 * in torch order -- rnn_layers.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, [.. _l1], output_layer.weight, .bias --
 * host or device memory, copied.  The hidden state of every lane is VS_POLICY_HIDDEN (zeroed here); per step and lane the
 * kernel computes act, h' = policy(obs, h) with torch's cell equations, records, steps, and carries h' to the next step and
 * launch.  desc == NULL removes the policy; setting one removes a network of vs_set_policy_fnn and the other way round.
 * Refused like vs_set_policy_fnn (wrapper pipeline VS_ERR_STATE, discrete family / sizes / limits VS_ERR_ARG). */
int vs_set_policy_rnn(vs_handle h, const vs_rnn_desc* desc, const float* params, int64_t n_params);
/* vs_step_policy with a linear policy on a feature stack (vs_lin_desc).  `params` is the policy's flat parameter vector in torch
 * order -- net.weight [A][F] row-major, F features in stack order -- host or device memory, copied (n_params = A * F).
 * desc == NULL removes the policy; setting a linear policy removes a policy of vs_set_policy_fnn / vs_set_policy_rnn and any
 * population, and the other way round.  vs_set_policy_population then takes sets of A * F floats each.  Records, auto-reset,
 * freeze-at-done and launch cuts as for vs_set_policy_fnn; vs_set_policy_shape has no meaning for a linear policy and is ignored.
 * Refused with the previous policy (and population) left in place: a wrapper pipeline on the handle (VS_ERR_STATE); the
 * discrete-action family, an unknown kind, an elementwise kind or VS_FEAT_CONST twice, an index outside the visible rows, a
 * MultFeat of fewer than 2 or more than 4 rows, more than VS_LIN_MAX_XTERMS / VS_LIN_MAX_FEAT terms / features, a negative or NaN
 * noise_std, n_params != A * F (VS_ERR_ARG). */
int vs_set_policy_linear(vs_handle h, const vs_lin_desc* desc, const float* params, int64_t n_params);
/* vs_step_policy with an open-loop policy that replays recorded actions: PlaybackPolicy (one recording per rollout) and, as a
 * tabulated function of time, TimePolicy of upstream Pyrado policies/feed_forward/playback.py and time.py.
 * `actions` is [n_rec][t_len][A] row-major, host or device memory, copied and re-laid on the device ([t_len][A][n_rec rounded up
 * to 64]); rec_len[n_rec] (host; NULL: every recording has t_len steps) the number of steps of each recording, 0 .. t_len;
 * lane_rec[n_envs] (host) the recording each lane replays, NULL: lane i replays (first_global_index + i) % n_rec
 * (vs_set_index_offset).  The action of a step of a lane with recording r, k = the env's curr_step BEFORE the step:
 *     act[j] = k < rec_len[r] ? actions[r][k][j] : 0
 * -- k is the env's own counter, so cutting a rollout into several launches does not show, and an auto-reset restarts the
 * recording with the episode.  The raw table value is what a record holds as the action; VS_FLAG_ACT_NORM, the clip and the dead
 * zone apply to it inside the step as for every other policy, NaN sets VS_ERRFLAG.  A lane frozen at done reads nothing (its
 * recorded action is 0).  noise_seed of vs_step_policy is ignored.  Records, auto-reset, freeze-at-done as for vs_set_policy_fnn.
 * actions == NULL removes the policy.  Setting a playback policy removes a policy of vs_set_policy_fnn / vs_set_policy_rnn /
 * vs_set_policy_linear, any population and any rollout target, and the other way round; vs_set_policy_population on a playback
 * policy returns VS_ERR_STATE.
 * Refused with the previous policy (population, target) left in place: a wrapper pipeline on the handle (VS_ERR_STATE); the
 * discrete-action family, n_rec < 1, t_len < 1, a rec_len outside [0, t_len], a lane_rec outside [0, n_rec), a table of more
 * than 2^31 floats (VS_ERR_ARG). */
int vs_set_policy_playback(vs_handle h, const float* actions, int n_rec, int t_len, const int32_t* rec_len, const int32_t* lane_rec);
/* The on-device trajectory discrepancy of a playback rollout (the inner loop of system identification: simulate a recorded
 * segment under candidate domain parameters, compare with the recorded observations) -- replaces recording, packing and
 * copying every step to evaluate  sum_k sum_d w_d (obs_sim[k][d] - obs_rec[k][d])^2  on the host.
 * target_obs is [n_rec][t_len + 1][O] row-major (host or device, copied and re-laid), row k = the recorded observation after k
 * steps (row 0, the initial observation, is not compared); weights[O] (host), NULL: all 1.  Setting a target allocates
 * VS_ROLLOUT_LOSS and zeroes it; vs_reset zeroes it for the lanes it resets.  vs_step_policy then, after every step a
 * non-frozen lane with recording r takes, k' = its new curr_step, if k' <= rec_len[r]:  for d = 0 .. O - 1, in that order, in fp32
 *     e = obs'[d] - target_obs[r][k'][d];   VS_ROLLOUT_LOSS[lane] = fmaf(weights[d] * e, e, VS_ROLLOUT_LOSS[lane])
 * (obs' the observation of the new state).  The number of steps in a lane's sum is min(VS_STEPCOUNT, rec_len[r]).  With
 * record == 0 such a launch writes nothing per step.
 * target_obs == NULL removes the target; replacing or removing the playback policy removes it too.
 * Refused: no playback policy on the handle (VS_ERR_STATE); n_rec / t_len different from the playback policy's, a negative or
 * NaN weight (VS_ERR_ARG).  With a target and auto-reset on, vs_step_policy returns VS_ERR_STATE. */
int vs_set_rollout_target(vs_handle h, const float* target_obs, int n_rec, int t_len, const float* weights);
/* Sensitivities of the trajectory discrepancy with respect to domain parameters (gradient-based identification: Gauss-Newton,
 * Levenberg-Marquardt): vs_step_policy on a handle with a playback policy and a rollout target then runs a kernel that, next
 * to VS_ROLLOUT_LOSS (the same bits, as are state, hidden state, observation, flags and step counter), carries
 * d (state, hidden state) / d theta_j from step to step in forward mode for the n_params chosen parameters theta_j =
 * vs_param_name(type, param_idx[j]) and sums, where the loss sums a step, with e_d the loss's own e and J_dj = d obs'[d] / d theta_j,
 * for d = 0 .. O - 1 in that order, in fp32
 *     VS_ROLLOUT_GRAD[j][lane]   = fmaf(2 weights[d] e_d, J_dj, VS_ROLLOUT_GRAD[j][lane])
 *     VS_ROLLOUT_GN[(j,l)][lane] = fmaf(weights[d] J_dj, J_dl, VS_ROLLOUT_GN[(j,l)][lane])      (j <= l, upper triangle, row-major)
 * The derivative runs through _calc_constants and the dynamics on the lane's own VS_PARAMS; the bounds of the action and state
 * spaces, the initial state and the initial hidden state are held constant with respect to the parameters, and kinks (clip,
 * dead zone, Coulomb friction's sign) follow the branch taken.  A lane frozen at done adds nothing; a lane that ends early stops
 * summing at its last step, like the loss.  The kernel carries NP = 1, 2 or 4 tangents: n_params = 3 runs 4 with an unseeded
 * column.  All three buffers are zeroed by this call and by vs_set_rollout_target (every lane) and by vs_reset (the reset
 * lanes); they carry over launch cuts.  n_params == 0 (param_idx may be NULL) turns the sensitivities off and frees the
 * buffers; vs_set_policy_fnn / _rnn / _linear / _playback drop them with the playback policy, removing the target drops them too.
 * With sensitivities on, vs_step_policy with record != 0 returns VS_ERR_STATE (recorded rollouts come from the plain kernel:
 * the same values).
 * Refused with the handle left as it was: NULL param_idx with n_params > 0, n_params outside 0 .. VS_SENS_MAX_PARAMS, an index
 * outside the family's parameter list or repeated (VS_ERR_ARG); no playback policy or no rollout target on the handle,
 * auto-reset on, a wrapper pipeline on the handle, the discrete-action family (VS_ERR_STATE). */
#define VS_SENS_MAX_PARAMS 4
int vs_set_rollout_sens(vs_handle h, const int32_t* param_idx, int n_params);
/* Reverse-mode gradients through recorded rollouts: the vector-Jacobian product of rows 0 .. t_steps - 1 of VS_TRAJ_REC (record mode
 * 2: row t holds the state s_t, the hidden state h_t and the raw action a_t before step t) with respect to every action and the
 * initial state, in one backward sweep -- what a T-step shooting method, an initial-state estimate or any loss written over the
 * observations and rewards of a rollout needs of the simulator.  (vs_step_jac has the one-step Jacobians, with the hidden state
 * held constant; vs_set_rollout_sens the forward form for domain parameters.)  The records may come from any recording path with
 * auto-reset off, started at a reset: vs_step_policy, vs_step_random or vs_step_record.  All pointers are device f32 owned by the
 * caller, ld = vs_ld(h); the call runs on the handle's stream and writes nothing but d_act and d_init: no state, reward or flag,
 * the handle's running state is untouched.
 *   g_rew         [t_steps][ld]         cotangent of the reward of step t; NULL: 0
 *   g_obs         [t_steps + 1][O][ld]  cotangent of the observation after k steps, row k (row 0: the initial observation); NULL: 0
 *   g_state_last  [S + H][ld]           cotangent of the state and hidden state after the lane's last step; NULL: 0
 *   d_act         [t_steps][A][ld]      out: d Phi / d a_t
 *   d_init        [S + H][ld]           out: d Phi / d (s_0, h_0)
 * with Phi = sum_t g_rew[t] r_t + sum_k g_obs[k] . obs_k + g_state_last . (s_L, h_L) per lane.  The lane's length is
 * L = min(t_steps, 1 + first row whose VS_TRAJ_DONE bit is set); lanes >= n_envs have L = 0 and get zeros.  lambda [S + H] starts as
 * g_state_last; for t = L - 1 .. 0 the step code itself (step_one and observe on dual numbers: step counter t, the final reward not
 * yet paid, the lane's stored constants) is differentiated at x = (s_t, h_t, a_t) and, for every column k of x, in fp32 in this order
 *     acc = 0;  for j < S: acc = fmaf(lambda[j], d s'_j / d x_k, acc);  for j < H: acc = fmaf(lambda[S + j], d h'_j / d x_k, acc);
 *     acc = fmaf(g_rew[t], d r / d x_k, acc);  for q < O: acc = fmaf(g_obs[t + 1][q], d obs'_q / d x_k, acc)
 * The columns of (s, h) are the new lambda, those of a are d_act[t].  After t = 0, lambda[k] = fmaf(g_obs[0][q], d observe(s_0)_q /
 * d s_k, lambda[k]) for q < O, and d_init = lambda.  Rows t >= L of d_act are written 0; cotangent rows behind a lane's end are not
 * read (g_obs rows 0 .. L, g_rew rows 0 .. L - 1 are).
 * Conventions, as for vs_step_jac and vs_set_rollout_sens: the raw action is the differentiation variable -- ActNormWrapper's map,
 * the clip and the dead zone are inside the step and kinks follow the branch taken, so nothing reaches the dynamics through a
 * clipped action (the reward's action cost is a function of the unclipped action and keeps its term); domain parameters and the
 * bounds of the spaces are constants.  Unlike vs_step_jac the hidden state (qcp: th_ddot, qbb: plate angles) is part of the adjoint.
 * Refused with nothing written: NULL handle, d_act or d_init, t_steps < 1 or beyond vs_set_traj_capacity (VS_ERR_ARG); record mode
 * other than 2, auto-reset on, a wrapper pipeline on the handle, a trajectory offset other than 0 (vs_set_traj_offset), the
 * discrete-action family (VS_ERR_STATE). */
int vs_rollout_vjp(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_state_last, float* d_act,
                   float* d_init);
/* The same sweep with the gradient with respect to DOMAIN PARAMETERS next to it: for the n_params chosen parameters theta_j =
 * vs_param_name(type, param_idx[j]) of every lane's own VS_PARAMS,
 *   d_params  [n_params][ld]   out: d Phi / d theta_j, Phi as for vs_rollout_vjp
 * -- what system identification by gradient needs of the simulator for ANY loss written over the observations of a recorded rollout
 * (vs_set_rollout_sens has the forward form, for the weighted squared discrepancy against a target table only).  Arguments, layout
 * (ld = vs_ld(h)), stream, L, the NULL-is-zero rule of the cotangents and "writes nothing of the handle" are vs_rollout_vjp's, and
 * d_act and d_init are vs_rollout_vjp's bit for bit.  n_params is 1 .. VS_SENS_MAX_PARAMS; the kernel carries NP = 1, 2 or 4
 * tangents, n_params = 3 runs 4 with an unseeded column.  As in vs_set_rollout_sens the tangents run through _calc_constants on
 * the lane's raw parameters (the constants' values are the lane's stored ones) and the dynamics.  dp[j] = 0; then for t = L - 1 .. 0,
 * BEFORE lambda is updated (it holds the adjoint of (s_{t+1}, h_{t+1})), the dynamics and observe are differentiated at the recorded
 * (s_t, h_t) and the applied action (ActNormWrapper's map and the clip in float: constants) and, for every j, in fp32 in this order
 *     for k < S: dp[j] = fmaf(lambda[k], d s'_k / d theta_j, dp[j]);  for k < H: dp[j] = fmaf(lambda[S + k], d h'_k / d theta_j, dp[j]);
 *     for q < O: dp[j] = fmaf(g_obs[t + 1][q], d obs'_q / d theta_j, dp[j])
 * then the step of vs_rollout_vjp.  d_params[j] = dp[j]; lanes >= n_envs get 0.  Cotangent rows behind a lane's end are not read.
 * Conventions, as for vs_set_rollout_sens: the reward, the bounds of the action and state spaces, the clip, the initial state and the
 * initial hidden state are constants with respect to the parameters -- g_rew and g_obs[0] add nothing to d_params --, and kinks
 * (clip, dead zone, Coulomb friction's sign) follow the branch taken.  More than VS_SENS_MAX_PARAMS parameters are further calls
 * over the same records.
 * Refused with nothing written: everything vs_rollout_vjp refuses, with the same codes; NULL d_params or param_idx, n_params outside
 * 1 .. VS_SENS_MAX_PARAMS, an index outside the family's parameter list or repeated (VS_ERR_ARG). */
int vs_rollout_vjp_params(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_state_last,
                          const int32_t* param_idx, int n_params, float* d_act, float* d_init, float* d_params);
/* The same sweep for CLOSED-LOOP rollouts: rows 0 .. t_steps - 1 were recorded by vs_step_policy with the handle's current linear
 * policy (vs_set_policy_linear) in the loop, a_t = W phi(obs_t) + n_t, where n_t -- the exploration noise, if any -- is a constant the
 * recorded raw action already contains.  The caller answers for the policy on the handle being the one that made the records.
 * Per lane the differentiated function is
 *     Phi = sum_t g_rew[t] r_t + sum_k g_obs[k] . obs_k + sum_t g_act[t] . a_t + g_state_last . (s_L, h_L)
 * of that closed loop, L and every convention as for vs_rollout_vjp.  Arguments, layout (ld = vs_ld(h)), stream and the rule "refused
 * before the first device call, outputs untouched" are vs_rollout_vjp's, with one more cotangent:
 *   g_act   [t_steps][A][ld]   cotangent of the raw policy action a_t; NULL: 0
 *   d_act   [t_steps][A][ld]   out: the TOTAL adjoint abar_t of a_t = d Phi / d n_t -- what the policy's parameter gradient needs:
 *                              d Phi / d W = sum_t abar_t phi(obs_t)^T over the recorded observations (left to the caller: one GEMM,
 *                              or vs_lin_param_grad below, one device pass over the handle's own records)
 *   d_init  [S + H][ld]        out: d Phi / d (s_0, h_0), feedback through the policy included
 * For t = L - 1 .. 0 the step is differentiated as in vs_rollout_vjp with the observation cotangent g_obs[t + 1] + gpol, gpol [O] being
 * the policy's pull-back of step t + 1 (0 at t = L - 1; observe(s_{t+1}) is the observation the policy saw);  abar_t = (the step's
 * action column) + g_act[t];  gpol = (d phi / d obs)(obs_t)^T W^T abar_t with obs_t = observe(s_t) of the recorded state and the
 * derivatives of the feature functions as the rollout kernel evaluates them (sign, const: 0; |v|: sign(v), 0 at 0; MultFeat: product
 * rule per position; ATan2Feat(y, x): (x, -y) / (x^2 + y^2)).  After t = 0 the initial observation takes g_obs[0] + gpol.
 * With a stack of constant features the result equals vs_rollout_vjp's bit for bit.
 * Refused with nothing written: everything vs_rollout_vjp refuses, with the same codes; no linear policy on the handle (an FNN, RNN
 * or playback policy, or none) and a policy population on the handle (VS_ERR_STATE).  Feed-forward networks have vs_rollout_vjp_fnn, recurrent policies vs_rollout_vjp_rnn. */
int vs_rollout_vjp_policy(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_act,
                          const float* g_state_last, float* d_act, float* d_init);
/* ... and for rollouts recorded with the handle's current FEED-FORWARD NETWORK (vs_set_policy_fnn) of one or two hidden layers in the
 * loop: a_t = g(W_out f(.. f(W_1 x_t + b_1) ..) + b_out) + n_t, x_t = the observation rows the policy sees (obs_idx), optionally in the
 * featurisation [o_0, sin o_1, cos o_1, o_2 ..], n_t constant.  Phi, arguments, layout (ld = vs_ld(h)), stream, L, every convention and
 * the rule "refused before the first device call, outputs untouched" are vs_rollout_vjp_policy's; d_act is again the TOTAL adjoint
 * abar_t of the raw action a_t (the output nonlinearity's own derivative is applied only on the way to gpol), so that
 * d Phi / d theta = sum_t (d pi / d theta)(obs_t)^T abar_t is one batched backward pass of the network over the recorded observations,
 * left to the caller.  Per step the activations of obs_t = observe(s_t) are recomputed with the rollout kernel's expressions (the
 * summation order differs, as it does between the rollout kernel's own shapes) and pulled back:
 *     delta_out = abar_t (.) g'(y_out);  delta_l = (W_{l+1}^T delta_{l+1}) (.) f'(y_l);  gx = W_1^T delta_1
 * with tanh' = 1 - y^2, sigmoid' = y (1 - y), relu' = [y > 0] (0 at 0), none: 1;  under the featurisation o_1 takes
 * gx_1 cos o_1 - gx_2 sin o_1;  gpol is gx on the observation rows obs_idx names.  Rows t >= L and lanes >= n_envs contribute nothing
 * and get zeros, whatever the records hold there.
 * Refused with nothing written: everything vs_rollout_vjp refuses, with the same codes; no feed-forward network on the handle (a
 * linear, RNN or playback policy, or none), a policy population on the handle, a network of more than two hidden layers (its weights
 * and their transposes do not fit the register file) (VS_ERR_STATE). */
int vs_rollout_vjp_fnn(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_act,
                       const float* g_state_last, float* d_act, float* d_init);
/* The parameter gradient that vs_rollout_vjp_fnn leaves to the caller, as one device pass over the same records:
 *     d Phi / d theta = sum over the rows t < L of every lane i < n_envs of (d pi / d theta)(x_t)^T abar_t
 * for the handle's current feed-forward network of one or two hidden layers, i.e. per row
 *     dW_out += delta_out y_last^T, db_out += delta_out;  dW_l += delta_l y_{l-1}^T, db_l += delta_l  (y_0 = x_t)
 * with delta_out = abar_t (.) g'(y_out), delta_l = (W_{l+1}^T delta_{l+1}) (.) f'(y_l) and the activations recomputed with the rollout
 * kernel's expressions, as in vs_rollout_vjp_fnn.  x_t is built from the RECORDED observation of row t (obs_idx, featurisation): the
 * row the policy saw.  L is the lane's length as vs_rollout_vjp takes it from the done bits of rows 0 .. t_steps - 1.
 *   abar      [t_steps][A][ld]   device: d_act as vs_rollout_vjp_fnn returned it (ld = vs_ld(h)).  Rows t >= L, lanes >= n_envs and
 *                                anything behind row t_steps are never read into the arithmetic: they may hold anything, NaN included
 *   d_params  [n_params]         device, out: the gradient in the order of the parameter vector vs_set_policy_fnn took (per Linear
 *                                weight [out][in], then bias); accumulate != 0: added to what is there, one fp32 add per entry
 * Runs on the handle's stream and writes nothing of the handle.  The sum is deterministic: no atomics, every partial sum is added in
 * a fixed order that depends on (ld, t_steps, device) only, so two calls on the same inputs return the same bits.  A workspace for
 * the partial sums belongs to the network on the handle: allocated at the first call, freed when the policy is replaced or removed.
 * Refused with nothing written: everything vs_rollout_vjp_fnn refuses, with the same codes; NULL abar or d_params, n_params other
 * than the network's parameter count (VS_ERR_ARG). */
int vs_fnn_param_grad(vs_handle h, int t_steps, const float* abar, float* d_params, int64_t n_params, int accumulate);
/* The weight gradient that vs_rollout_vjp_policy leaves to the caller, as one device pass over the same records:
 *     d Phi / d W[j][q] = sum over the rows t < L of every lane i < n_envs of abar_t[j] phi_q(x_t)
 * for the handle's current linear policy (vs_set_policy_linear), phi_q the q-th feature of its stack evaluated with the rollout
 * kernel's expressions (sincos_fast, v_exp_f32, the bare v_rcp_f32, the device library's atan2f).  x_t is built from the RECORDED
 * observation of row t (obs_idx): the row the policy saw.  L is the lane's length as vs_rollout_vjp takes it from the done bits of
 * rows 0 .. t_steps - 1.
 *   abar      [t_steps][A][ld]   device: d_act as vs_rollout_vjp_policy returned it (ld = vs_ld(h)).  Rows t >= L, lanes >= n_envs
 *                                and anything behind row t_steps are never read into the arithmetic: they may hold anything, NaN
 *                                included
 *   d_params  [A * F]            device, out: the gradient in the order of the parameter vector vs_set_policy_linear took (net.weight
 *                                [A][F] row-major, F features in stack order); accumulate != 0: added to what is there, one fp32 add
 *                                per entry
 * Runs on the handle's stream and writes nothing of the handle.  The sum is deterministic: no atomics, every partial sum is added in
 * a fixed order that depends on (ld, t_steps, device) only, so two calls on the same inputs return the same bits.  A workspace for
 * the partial sums belongs to the policy on the handle: allocated at the first call, freed when the policy is replaced or removed.
 * Refused with nothing written: everything vs_rollout_vjp_policy refuses, with the same codes; NULL abar or d_params, n_params
 * other than the policy's parameter count, more than 2^31 - 1 tiles of 64 lanes x one step (VS_ERR_ARG). */
int vs_lin_param_grad(vs_handle h, int t_steps, const float* abar, float* d_params, int64_t n_params, int accumulate);
/* ... and for rollouts recorded with the handle's current RECURRENT policy (vs_set_policy_rnn: RNN tanh / relu, GRU or LSTM of one or
 * two layers) in the loop: (a_t, p_{t+1}) = F(x_t, p_t) + (n_t, 0), p the packed hidden state [Hs] (h of layer 0, 1, .. then, LSTM, c
 * of layer 0, 1, ..), x_t the observation rows the policy sees (obs_idx), n_t constant.  The differentiated function is
 *     Phi = sum g_rew r + sum g_obs obs + sum g_act a + g_state_last (s_L, h_L) + g_hid_last p_L
 * and TWO adjoints run backwards: the env's lambda [S + H] and the policy's eta [Hs].  Arguments, layout (ld = vs_ld(h)), stream, L and
 * the NULL-is-zero rule of the cotangents are vs_rollout_vjp_fnn's; new: g_hid_last [Hs][ld] (NULL = 0), d_hid [t_steps][Hs][ld] and
 * d_hid0 [Hs][ld] (either may be NULL: not written).  d_act[t] is the total adjoint abar_t of the raw action; d_hid[t] is the TOTAL
 * cotangent of p_{t+1} -- everything downstream of step t, g_hid_last at t = L - 1, step t's own output layer not included --, so that
 *     d Phi / d theta = sum_t (d F / d theta)(x_t, p_t)^T (abar_t, d_hid[t])
 * is one batched single-step backward pass of the policy over the recorded observations and hidden states (row t of
 * VS_POLICY_HIDDEN_REC is p_t), left to the caller.  d_hid0 is the cotangent of p_0, d_init includes the feedback through the policy.
 * Per step the cell is recomputed at the recorded (x_t, p_t) with the rollout kernel's expressions and pulled back with the derivatives
 * of the functions that ran (tanh 1 - y^2, sigmoid y (1 - y), relu [y > 0]).  Rows t >= L of d_act and d_hid and lanes >= n_envs get
 * zeros and read no cotangent.
 * Refused with nothing written: everything vs_rollout_vjp refuses, with the same codes; no recurrent policy on the handle (an FNN,
 * linear or playback policy, or none), a policy population on the handle, no hidden-state record plane or one whose width differs from
 * the policy's Hs (VS_ERR_STATE). */
int vs_rollout_vjp_rnn(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_act,
                       const float* g_state_last, const float* g_hid_last, float* d_act, float* d_init, float* d_hid, float* d_hid0);
/* The parameter gradient that vs_rollout_vjp_rnn leaves to the caller, as one device pass over the same records:
 *     d_params[q] = sum over the rows t < L of every lane i < n_envs of (d F / d theta_q)(x_t, p_t)^T (abar_t, d_hid[t])
 * for the handle's current recurrent policy (all four cells, one or two layers), i.e. per row and layer
 *     dW_ih += delta x^T, dW_hh += delta h^T, db_ih += delta, db_hh += delta;   dW_out += delta_out h'_top^T, db_out += delta_out
 * with the gates recomputed at the recorded (x_t, p_t) with the rollout kernel's expressions and the deltas formed as in
 * vs_rollout_vjp_rnn (GRU: W_hn and b_hn take delta_n r, W_in and b_in delta_n; LSTM: the cell adjoint is d_hid's c part; two layers:
 * the adjoint of layer 0's h' is its d_hid part plus layer 1's W_ih^T delta).  x_t is the RECORDED observation of row t through obs_idx,
 * p_t row t of VS_POLICY_HIDDEN_REC, L the lane's length as vs_rollout_vjp takes it.
 *   abar      [t_steps][A][ld]    device: d_act as vs_rollout_vjp_rnn returned it (ld = vs_ld(h))
 *   d_hid     [t_steps][Hs][ld]   device: d_hid as vs_rollout_vjp_rnn returned it.  Of both, and of the hidden-state record, rows
 *                                 t >= L, lanes >= n_envs and anything behind row t_steps are never read into the arithmetic: they
 *                                 may hold anything, NaN included
 *   d_params  [n_params]          device, out: the gradient in the order of the parameter vector vs_set_policy_rnn took;
 *                                 accumulate != 0: added to what is there, one fp32 add per entry
 * Runs on the handle's stream and writes nothing of the handle.  The sum is deterministic: no atomics, every partial sum is added in
 * a fixed order that depends on (ld, t_steps, device) only, so two calls on the same inputs return the same bits.  A workspace for
 * the partial sums belongs to the policy on the handle: allocated at the first call, freed when the policy is replaced or removed.
 * Refused with nothing written: everything vs_rollout_vjp_rnn refuses, with the same codes; NULL abar, d_hid or d_params, n_params
 * other than the policy's parameter count, more than 2^31 - 1 tiles of 64 lanes x one step (VS_ERR_ARG). */
int vs_rnn_param_grad(vs_handle h, int t_steps, const float* abar, const float* d_hid, float* d_params, int64_t n_params, int accumulate);
/* The closed-loop sweep for a handle with a policy POPULATION (vs_set_policy_population) of linear policies or of feed-forward
 * networks of one or two hidden layers; it dispatches on the policy slot.  Every lane's sweep runs with the weights of the set its
 * aligned group of 64 lanes names -- the statements of vs_rollout_vjp_policy / vs_rollout_vjp_fnn on that set's packed vector.
 * Arguments, layouts (ld = vs_ld(h)), the NULL-is-zero rule of the cotangents, the stream and "writes nothing of the handle" are
 * vs_rollout_vjp_policy's.  The lanes of an inert group (set -1) have L = 0 whatever their done bits hold, as vs_rollout_lengths has
 * it: zero rows of d_act, a zero d_init, no record and no cotangent read.
 * Refused with nothing written: everything vs_rollout_vjp refuses, with the same codes; no population on the handle, a recurrent or
 * playback policy (or none), a network of more than two hidden layers (VS_ERR_STATE).  The single-policy sweeps keep refusing a
 * handle with a population; a population of recurrent policies has no sweep. */
int vs_rollout_vjp_pop(vs_handle h, int t_steps, const float* g_rew, const float* g_obs, const float* g_act,
                       const float* g_state_last, float* d_act, float* d_init);
/* The parameter gradients that vs_rollout_vjp_pop leaves to the caller, one row per member, as one device pass over the same records:
 *     d_params[s][q] = sum over the rows t < L of the lanes i < n_envs whose group names set s of (d a_t / d theta_q)^T abar_t
 * with the terms of vs_lin_param_grad (linear) or vs_fnn_param_grad (network, evaluated with set s's weights).
 *   abar      [t_steps][A][ld]      device: d_act as vs_rollout_vjp_pop returned it.  Rows t >= L, lanes >= n_envs, inert groups and
 *                                   anything behind row t_steps are never read: they may hold anything, NaN included
 *   d_params  [n_sets][n_params]    device, out: row s in the order of the parameter vector the policy's setter took (net.weight for a
 *                                   linear policy, parameters_to_vector for a network).  A set that no group names gets zeros.
 *                                   accumulate != 0: added to what is there, one fp32 add per entry; an unnamed set's row is left alone
 * Runs on the handle's stream and writes nothing of the handle.  Deterministic: no atomics; a workgroup serves exactly one set, the
 * partition of the tile space among the sets and the order of every sum depend on (lane table, t_steps, device) only, so two calls on
 * the same inputs return the same bits.  The workspace is the policy slot's, the partition tables are kept with the population.
 * Refused with nothing written: everything vs_rollout_vjp_pop refuses, with the same codes; NULL abar or d_params, n_sets other than
 * the population's, n_params other than the policy's parameter count, more than 2^31 - 1 tiles of 64 lanes x one step (VS_ERR_ARG). */
int vs_pop_param_grad(vs_handle h, int t_steps, const float* abar, float* d_params, int n_sets, int64_t n_params, int accumulate);
/* The partition vs_pop_param_grad derives for a lane table, on the host alone (no handle, no device): groups [n_groups] is the set of
 * every aligned group of 64 lanes (-1: inert or past n_envs), per_wg the waves of a workgroup (1 linear, 4 network), cap the grid cap of
 * the single-policy pass (4 x / 2 x the compute units).  Writes seg [n_sets][2] = {first workgroup, workgroups} of every set and, where
 * given, wg [n_wg][4] = {first entry of the set, its entries, rank, workgroups of the set} (only if n_wg <= wg_cap) and ent (at most
 * n_groups entries: the groups that name a set, in stable order by (set, group)).  Returns the number of workgroups, or VS_ERR_ARG
 * (negative) for a NULL table or seg, counts below 1, a set id outside -1 .. n_sets - 1 or more than 2^31 - 1 tiles. */
int vs_pop_partition(const int32_t* groups, int n_groups, int n_sets, int t_steps, int per_wg, int64_t cap, int32_t* seg, int32_t* wg,
                     int wg_cap, int32_t* ent);
/* The gradient of the exploration noise's std that the three closed-loop sweeps leave out, as one device pass.  The policy kernels
 * form the raw action as a_t = mean_t + noise_std (.) eps_t (NormalActNoiseExplStrat, P/exploration/stochastic_action.py:121-180:
 * the reparameterised sample of Normal(mean, std)), eps_t ~ N(0, 1) keyed by (noise_seed, index offset + lane, episode, step), and
 * the sweeps return the TOTAL adjoint abar_t of the raw action as d_act, so
 *     d Phi / d noise_std[j] = sum over the rows t < L of every lane i < n_envs of abar_t[j] eps_t[j].
 * eps is not stored anywhere: it is drawn again with the rollout kernels' own calls and is their noise bit for bit -- the noise a
 * recording vs_step_policy(.., noise_seed) adds to rows 0 .. t_steps - 1 of a record that starts at a reset (step counter 0 at row 0,
 * in one launch or several; the episode counter is the handle's current one).  A policy set with noise_std = 0 is served: eps is
 * defined by the key alone, it is the noise a launch with this noise_seed WOULD add, and the derivative at 0 is the same sum.
 *   abar        [t_steps][A][ld]  a sweep's d_act as written (lanes last); behind a lane's end and at lanes >= n_envs it is never read
 *   d_std       [A], device       out: the gradient; accumulate != 0: added to what it holds, one fp32 add per entry
 *   d_std_lane  [A][ld] or NULL   out: every lane's own sum over t (in increasing t), 0 at lanes >= n_envs
 *   eps         [t_steps][A][ld] or NULL   out: the regenerated noise, exact zeros behind a lane's end and at lanes >= n_envs
 * Runs on the handle's stream and writes nothing of the handle.  Deterministic, no atomics: a partial sum per workgroup, then one
 * reduction in a fixed order; the grid is a function of (ld, t_steps, device), so two calls return the same bits.  The workspace
 * belongs to the policy on the handle: allocated at the first call, freed when the policy is replaced or removed.
 * Accepted: a handle with a linear, feed-forward or recurrent policy and the records of record mode 2.  Refused with nothing
 * written: everything vs_rollout_vjp refuses, with the same codes; no policy, a playback policy, a population (VS_ERR_STATE); NULL
 * abar or d_std -- both (and d_std_lane) may be NULL only together, with eps given: the eps-only call --, more than 2^31 - 1 tiles
 * of 64 lanes x one step (VS_ERR_ARG). */
int vs_noise_std_grad(vs_handle h, int t_steps, uint64_t noise_seed, const float* abar, float* d_std, int accumulate,
                      float* d_std_lane, float* eps);
/* the hidden-state record plane VS_POLICY_HIDDEN_REC: width floats per env and recorded step (0 = off, the default: no traffic).
 * A recording vs_step_policy with a recurrent policy fills it when width equals the policy's packed hidden size. */
int vs_set_policy_hidden_record(vs_handle h, int width);
/* the policy-in-the-loop counterpart: the caller's hidden state (device f32, element (env i, unit j) at
 * hidden[i * env_stride + j * dim_stride], width units) into row `row` of VS_POLICY_HIDDEN_REC; row < 0: the device-side
 * counter of vs_step_record, NOT advanced -- call it before the vs_step_record of the same step (captured graphs replay it) */
int vs_record_hidden(vs_handle h, const float* hidden, int64_t env_stride, int64_t dim_stride, int row);
/* A population for vs_step_policy: n_sets parameter vectors of the policy last set by vs_set_policy_fnn / vs_set_policy_rnn /
 * vs_set_policy_linear
 * (same architecture; vector s at params + s * n_params, each laid out like that call's `params`; host or device memory,
 * copied and packed on the device).  lane_set[i] (host, n entries) = the set lane i runs, or -1: the lane takes no part.
 * params == NULL removes the population (the single policy of the last vs_set_policy_* call applies again).
 * Every aligned group of 64 lanes names one set or is all -1 (VS_ERR_ARG otherwise; also for a wrong n_params or a set id
 * >= n_sets); without a policy VS_ERR_STATE.  The 256-env shapes of vs_set_policy_shape need every aligned group of 256 lanes
 * to name one set: the automatic choice falls back to shape 0, a pinned shape 1 or 2 makes vs_step_policy return
 * VS_ERR_STATE.  With a population vs_step_policy records (record != 0) and runs with auto-reset off (VS_ERR_STATE
 * otherwise); it leaves the -1 lanes alone -- no step, no record row written -- and vs_rollout_lengths reports 0 for them
 * (also after a vs_reset).  vs_set_policy_fnn / vs_set_policy_rnn / vs_set_policy_linear (a NULL desc included) remove the population. */
int vs_set_policy_population(vs_handle h, const float* params, int64_t n_params, int n_sets, const int32_t* lane_set);
/* The recorded steps of lanes 0 .. n_lanes - 1 (rows 0 .. of VS_TRAJ_REC, vs_set_record_mode's layout) as ROLLOUTS in one row-major
 * matrix rows[total + n_lanes][F] (F = vs_traj_layout's record width, device memory): rollout j = steps 0 .. lengths[j] - 1 of
 * lane j, the rollouts one after the other, starts[j] = lengths[0] + .. + lengths[j - 1] (both int64, device memory).
 *   rows[starts[j] + j + t]          the record of step t: [obs (O) | act (A) | rew | state (S) | act_app (A) | hidden (H)] (the last
 *                                    three in record mode 2 only), t < lengths[j];
 *   rows[starts[j] + j + lengths[j]] the entry behind the last step: final observation / state / hidden state from VS_OBS / VS_STATE /
 *                                    VS_HIDDEN of the lane (frozen at its done), the per-step fields 0.
 * Every field of a rollout is therefore a strided view of lengths[j] (per-step fields) or lengths[j] + 1 rows (observations, states,
 * hidden states: the value before every step and the final one).  Runs on the handle's stream.
 * Replaces: the histories rollout() returns per env -- P/sampling/rollout.py:305-325 (obs_hist / act_hist / rew_hist / state_hist /
 * act_app_hist / th_ddot_hist -> StepSequence) -- and their concatenation over rollouts, P/sampling/step_sequence.py:777-825. */
/* Where the rollouts in the records end: lengths[j] = 1 + the first of rows 0 .. t_steps - 1 of VS_TRAJ_DONE whose done bit is set
 * for lane j (t_steps if none is), done_last[j] = whether one is -- the step at which rollout()'s loop stops
 * (`while not done and env.curr_step < env.max_steps`, P/sampling/rollout.py:185) and StepSequence.done[-1].  Device memory. */
int vs_rollout_lengths(vs_handle h, int n_lanes, int t_steps, int64_t* lengths, uint8_t* done_last);
int vs_pack_traj(vs_handle h, int n_lanes, int t_steps, const int64_t* lengths, const int64_t* starts, float* rows);
/* Discounted reward-to-go and GAE advantages of packed rollouts: inside every rollout the recurrence y_t = x_t + c y_{t+1}, backwards
 * in time, as one segmented scan over the packed rows (three launches, no host synchronisation).  No handle: the packed rows belong
 * to the caller.  device_id / hip_stream: where to launch, a hipStream_t in vs_set_stream's convention (hipStreamLegacy = (hipStream_t)1
 * or NULL: the legacy default stream).  Everything else is device memory:
 *   n, lengths[n], starts[n]    as for vs_pack_traj (int64): rollout j has L = lengths[j] steps and base row b = starts[j] + j; the rows
 *                               b .. b + L - 1 are its steps, row b + L its final entry.  (A sub-range j0 .. of a batch: pass
 *                               lengths + j0, starts + j0 and the row pointers advanced by j0 rows.)
 *   rew, rew_stride             reward of step t of rollout j = rew[(b + t) * rew_stride] (the reward column of rows[total + n][F] where
 *                               it lies: rew_stride = F)
 *   values, values_stride       NULL, or a value estimate per packed row: row b + t = the value of the observation before step t, row
 *                               b + L that of the final observation (the rows of the packed observations)
 *   done_last[n]                NULL, or u8: the final value of the rollout does not bootstrap (it ended by failure; note that an
 *                               env's done flag is also set at the step limit -- VS_FAILED tells the two apart)
 *   out[total + n]              dense, on the same rows;  out_first[n] or NULL
 * With keep_j = done_last && done_last[j] ? 0 : 1, for t = L - 1 .. 0:
 *   VS_RETURNS_RETURN  y_L = values ? values[b + L] * keep_j : 0;   y_t = rew[b + t] + gamma * y_{t+1}
 *   VS_RETURNS_GAE     (values required)  V_L = values[b + L] * keep_j, V_t = values[b + t];  delta_t = rew[b + t] + gamma * V_{t+1} - V_t;
 *                      y_L = 0;   y_t = delta_t + gamma * lam * y_{t+1}      (Schulman et al. 2016, eq. 16)
 *   out[b + t] = y_t, out[b + L] = y_L, out_first[j] = y_0 (= y_L for L = 0: the inert lanes of a population).
 * A zero multiplier cuts: nothing behind a final-entry row reaches the rollout before it, a non-finite value stays in its rollout.
 * fp32 throughout; the summation order is fixed (two calls give the same bits) but is a tree, not the sequential order.
 * VS_ERR_ARG (before any device call; vs_last_error(NULL) names the reason): n <= 0, NULL lengths / starts / rew / out, VS_RETURNS_GAE
 * without values, an unknown mode, a stride < 1, gamma or lam outside [0, 1].  lengths must be >= 0 and starts their exclusive running sum.
 * Replaces: StepSequence.discounted_return, discounted_reverse_cumsum and gae_returns of P/sampling/step_sequence.py, over a
 * concatenation of rollouts. */
#define VS_RETURNS_RETURN 0
#define VS_RETURNS_GAE 1
int vs_returns_scan(int device_id, void* hip_stream, int64_t n, const int64_t* lengths, const int64_t* starts, const float* rew,
                    int64_t rew_stride, const float* values, int64_t values_stride, const uint8_t* done_last, float gamma, float lam,
                    int mode, float* out, float* out_first);
/* The action stream of vs_step_random is Philox(seed; global env index, absolute step index); the handle counts the
 * steps it has taken.  vs_seek_random repositions that counter (0 = start of a fresh batch of rollouts). */
int vs_seek_random(vs_handle h, uint64_t step_index);
/* rows of the VS_TRAJ_* buffers (grow-only; a larger capacity replaces and frees the previous buffers) */
int vs_set_traj_capacity(vs_handle h, int t_max);
/* what a recording vs_step_random writes per step: 1 = [obs | act | rew] (default), 2 = + [state | act_app | hidden], the
 * fields rollout() returns in its StepSequence (rollout.py:305-325).  Changing the mode drops the record buffers: set
 * the capacity again afterwards. */
int vs_set_record_mode(vs_handle h, int mode);
int vs_record_mode(vs_handle h);
/* rollout() stops stepping an env at done (rollout.py:185).  With freeze on (and auto-reset off) vs_step skips the lanes
 * whose VS_DONE flag is set: state, observation, step counter and flags stay, VS_REW reads 0, and whatever action such a
 * lane is fed cannot raise its NaN flag.  Off (default): env.step() after done keeps stepping, as in the reference. */
int vs_set_freeze_done(vs_handle h, int on);
/* SimPyEnv.step returns (obs, rew, done, info) and nothing else (P/environments/pysim/base.py:217-241).  vs_step by default also
 * keeps a running undiscounted return per env (VS_RETURNS, what the auto-reset books into VS_EPSTAT_RETSUM when an episode
 * ends) and the VS_FAILED byte: 9 bytes per env step on top of the 117 algorithmic ones of SURVEY.md 8(d).  With lean on,
 * vs_step reads and writes exactly that model: VS_RETURNS / VS_FAILED are left untouched (stale) and episodes that end under
 * auto-reset count into VS_EPSTAT_COUNT / VS_EPSTAT_LENSUM with a return of 0.  vs_step_random / vs_step_policy are not
 * affected (their returns live in registers).  Off by default. */
int vs_set_lean_step(vs_handle h, int on);
/* which kernel the next vs_step_random launches for this handle's configuration: 0 = k_rollout (one wave per 64 envs),
 * 1 = k_rollout_ws in 256-env workgroups, 2 = k_rollout_ws in 64-env workgroups (a physics wave and a reward/record wave
 * per 64 envs; chosen while the plain kernel would leave the SIMDs with a single wave, the small workgroups while the
 * batch cannot give every compute unit a large one).  Results are bit-identical. */
int vs_rollout_variant(vs_handle h);
/* pin the choice: -1 automatic (default), 0 k_rollout, 1 / 2 k_rollout_ws where the configuration allows it (no wrapper
 * pipeline, no state-and-time dependent final reward; a live randomizer / parameter buffer only for the families with
 * fixed action bounds and an unscaled reward: qq-*, qcp-su), else k_rollout */
int vs_set_rollout_variant(vs_handle h, int variant);
/* first row of the VS_TRAJ_* buffers written by the next recording vs_step_random (default 0): consecutive launches can
 * fill one long trajectory buffer, t0 + k_steps <= capacity */
int vs_set_traj_offset(vs_handle h, int t0);
/* Episode bookkeeping.  Always on: per-env accumulators VS_EPSTAT_* (plain per-lane adds, no atomics) -- what the
 * RCCL return gather reads.  Opt-in (vs_set_episode_log): every finished episode is also appended as (return, length,
 * env index) to the VS_EP_* ring, compacted with a wavefront ballot and one atomic per wave; that atomic is a shared
 * counter (about 90 appends/us chip-wide), so leave the log off on throughput runs with short episodes. */
int vs_set_episode_log(vs_handle h, int on);
int vs_clear_episodes(vs_handle h);

/* ---- mixed batches (BASELINE config 5): several env families stepped by ONE launch ----
 * A mixed handle groups up to 5 ordinary handles on one device (lanes sorted by type: each handle is one contiguous
 * segment).  A workgroup belongs to one segment, so the env-type dispatch is uniform per workgroup / wavefront.
 * Parameters, resets and data access go through the member handles; the mixed handle only fuses the launches.
 * vs_mixed_create (VS_ERR_ARG otherwise): 1..5 handles, each once, on one device, agreeing on auto-reset; it moves every
 * member onto the stream of the first.
 * A launch takes the auto-reset setting, the stream and -- vs_mixed_step_random -- the record mode from the first member, so it
 * refuses (VS_ERR_STATE) members that no longer agree on them: after vs_set_auto_reset or vs_set_record_mode on some members
 * only, or after vs_set_stream gave a member another stream than the first member's (its own resets and copies would no longer
 * be ordered with the launch; give every member the same stream again).  It also refuses a member that carries a wrapper
 * pipeline (vs_set_act_pipeline / vs_set_obs_pipeline) and a recording rollout whose traj offset + k_steps exceeds a member's
 * vs_set_traj_capacity; k_steps < 1 and action pointers that are not device memory are VS_ERR_ARG.  Every check comes before
 * any member changes: a refused launch moves no random stream and writes no buffer; vs_mixed_last_error names the cause. */
typedef struct vs_mixed* vs_mixed_handle;
int vs_mixed_create(const vs_handle* handles, int n, vs_mixed_handle* out);
int vs_mixed_destroy(vs_mixed_handle m);
const char* vs_mixed_last_error(vs_mixed_handle m);
/* vs_step_random / vs_step for every member in one kernel; actions[q] etc. are the arguments of vs_step for member q */
int vs_mixed_step_random(vs_mixed_handle m, uint64_t seed, int k_steps, int record);
int vs_mixed_step(vs_mixed_handle m, const float* const* actions, const int64_t* env_strides, const int64_t* dim_strides);
int vs_mixed_time_random(vs_mixed_handle m, uint64_t seed, int k_steps, int record, int iters, float* avg_ms);

/* ---- data access ---- */

void* vs_get(vs_handle h, int which);                       /* device pointer, NULL on error */
int vs_copy_to_host(vs_handle h, int which, void* dst);     /* whole buffer, pitch ld (synchronises the stream) */
int vs_copy_from_host(vs_handle h, int which, const void* src); /* VS_STATE / VS_HIDDEN / VS_STEPCOUNT: `state` setter */
/* number of lanes with the sticky error flag set (synchronises); the host shim raises pyrado.ValueErr when > 0 */
int64_t vs_error_count(vs_handle h);

/* ---- measurement ---- */

/* average device time [ms] of the step kernel over `iters` launches, measured with hipEvents on the handle's stream
 * (mode 0: vs_step with the given device actions, mode 1: vs_step_random(k_steps, record); recording launches rotate
 * through the record buffer in k_steps-row slots, so a capacity beyond the 256 MiB Infinity Cache makes it an HBM stream) */
int vs_time_step_kernel(vs_handle h, int mode, const float* actions, int64_t env_stride, int64_t dim_stride,
                        int k_steps, int record, int iters, float* avg_ms);
/* HIP-event stopwatch on the handle's stream: vs_timer_start records an event where the stream stands, vs_timer_stop
 * records a second one, waits for it and returns the device time between the two [ms] -- the time of exactly the launches
 * issued in between (bench.py brackets its timed region with it: kernel time and wall time of the same launches) */
int vs_timer_start(vs_handle h);
int vs_timer_stop(vs_handle h, float* ms);
/* streaming copy kernel (float4, 4 independent 16-B accesses per thread, non-temporal, one-shot grid, own stream) over
 * `bytes` of device memory: achieved GB/s read + write (in-repo HBM reference point) */
int vs_membw_probe(int device_id, int64_t bytes, int iters, float* gbps);
/* the same for a pure write stream (float4 stores): the ceiling of the record stream of vs_step_random */
int vs_memwrite_probe(int device_id, int64_t bytes, int iters, float* gbps);

#ifdef __cplusplus
}
#endif
#endif /* VECSIM_H */
