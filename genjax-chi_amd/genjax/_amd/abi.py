"""ctypes binding of include/gjx.h — the thin C-ABI layer between the Python host API and the
hand-written HIP kernels (libgjx_hip.so).

This module only declares structs/prototypes and checks status codes.  It never picks a library
by itself: `runtime.py` loads `lib/libgjx_hip.so` and fails loudly if it is missing.  (The test
suite loads the CPU oracle through the same class to drive the identical host logic on CPU
tensors; the product never does.)
"""

from __future__ import annotations

import collections
import ctypes as C
import os

c_u32p = C.POINTER(C.c_uint32)
c_u64p = C.POINTER(C.c_uint64)
c_f32p = C.POINTER(C.c_float)
c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_u8p = C.POINTER(C.c_uint8)

GJX_OK = 0
STATUS = {
    0: "GJX_OK",
    -1: "GJX_ERR_INVALID",
    -2: "GJX_ERR_UNSUPPORTED",
    -3: "GJX_ERR_WORKSPACE",
    -4: "GJX_ERR_LAUNCH",
    -5: "GJX_ERR_NO_DEVICE",
    -6: "GJX_ERR_JIT",
}

RNG_THREEFRY = 0
RNG_PHILOX = 1

LSE_RECORD_WORDS = 65  # include/gjx.h: GJX_LSE_RECORD_WORDS
DIST_NORMAL, DIST_GAMMA, DIST_BETA, DIST_BERNOULLI, DIST_CATEGORICAL = range(5)
ARG_CONST, ARG_SITE, ARG_INPUT, ARG_TABLE, ARG_STATE, ARG_OBS, ARG_PARAM, ARG_EXPR = range(8)
# postfix programs as distribution arguments (gjx.h: GJX_ARG_EXPR / gjx_expr_op)
(EXPR_CONST, EXPR_SITE, EXPR_INPUT, EXPR_PARAM, EXPR_STATE, EXPR_OBS, EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_NEG, EXPR_DIV, EXPR_EXP,
 EXPR_LOG, EXPR_SQRT, EXPR_ABS, EXPR_MAX, EXPR_MIN, EXPR_LT, EXPR_LE, EXPR_EQ, EXPR_SELECT) = range(21)
EXPR_UNARY = (EXPR_NEG, EXPR_EXP, EXPR_LOG, EXPR_SQRT, EXPR_ABS)
MAP_EXP, MAP_LOG, MAP_DIV, MAP_RDIV, MAP_SQRT, MAP_ABS = range(6)
MAX_EXPR_OPS, MAX_EXPR_DEPTH = 32, 8
MAX_PARAMS = 64
SMC_MAX_STATE, SMC_MAX_OBS = 4, 8
PATHS_MAX_COLS = SMC_MAX_STATE + 1  # gjx_paths.h: GJX_PATHS_MAX_COLS
PATHS_LEAVES_ORDERED = 1  # gjx_paths.h: GJX_PATHS_LEAVES_ORDERED
OP_LOGSUMEXP, OP_CATEGORICAL_INDEX, OP_RESAMPLE, OP_SMC = range(4)
MAX_SITES = 64
PLAN_FAST_MATH = 1  # gjx.h: GJX_PLAN_FAST_MATH


class GjxError(RuntimeError):
    def __init__(self, fn: str, code: int):
        super().__init__(f"{fn} failed: {STATUS.get(code, code)}")
        self.code = code


class HeaderUnavailable(GjxError):
    """An entry point of an optional header called on a library that does not export it (GJX_ERR_UNSUPPORTED)."""
    header = why = ""

    def __init__(self, fn: str, backend: str):
        RuntimeError.__init__(self, f"{fn}: the library '{backend}' does not implement include/{self.header} "
                                    f"(libgjx_hip.so does; {self.why})")
        self.code = -2


class PathsUnavailable(HeaderUnavailable):
    header, why = "gjx_paths.h", "the trace-back kernel has no CPU restatement"


class GuidedUnavailable(HeaderUnavailable):
    header, why = "gjx_guided.h", "the CPU oracle knows no proposed / guided sites and would misread their tables"


class BacksimUnavailable(HeaderUnavailable):
    header, why = "gjx_backsim.h", "backward simulation runs as generated HIP kernels only"


class BackmoveUnavailable(HeaderUnavailable):
    header, why = "gjx_backmove.h", "the MCMC backward moves run as generated HIP kernels only"


class SmcParamsUnavailable(HeaderUnavailable):
    header, why = "gjx_smc_params.h", "parameterised filters run as generated HIP kernels only"


class CsmcUnavailable(HeaderUnavailable):
    header, why = "gjx_csmc.h", "the conditional step runs as generated HIP kernels only"


class TemperUnavailable(HeaderUnavailable):
    header, why = "gjx_temper.h", "the tempered move runs as a generated HIP kernel only"


class PlateUnavailable(HeaderUnavailable):
    header, why = "gjx_plate.h", "plated likelihoods run inside the generated tempered move kernel only"


class PointwiseUnavailable(HeaderUnavailable):
    header, why = "gjx_pointwise.h", "pointwise predictive densities run as a generated HIP kernel over a plated plan only"


class PsisUnavailable(HeaderUnavailable):
    header, why = "gjx_psis.h", "PSIS-LOO runs as a generated HIP kernel over a plated plan only"


class PredictiveUnavailable(HeaderUnavailable):
    header, why = "gjx_predictive.h", "posterior predictive draws run as a generated HIP kernel over a plated plan only"


class CountsUnavailable(HeaderUnavailable):
    header, why = "gjx_counts.h", "the Poisson and negative-binomial densities and samplers are HIP kernels only"


class GroupUnavailable(HeaderUnavailable):
    header, why = "gjx_group.h", "grouped latents live in the generated tempered move kernel only"


class GroupChecksUnavailable(HeaderUnavailable):
    header, why = "gjx_group_checks.h", "the pointwise, PSIS and predictive kernels of a grouped plan are generated HIP kernels only"


class TemperCovUnavailable(HeaderUnavailable):
    header, why = "gjx_temper_cov.h", "the population moments and the covariance move run as HIP kernels only"


class Keys(C.Structure):
    _fields_ = [
        ("impl", C.c_int32),
        ("mode", C.c_int32),
        ("keys", C.c_void_p),
        ("parent", C.c_uint32 * 2),
        ("first", C.c_uint64),
        ("has_fold", C.c_int32),
        ("fold", C.c_uint32),
        ("parent_lane", C.c_uint64),
    ]


class Scope(C.Structure):
    """include/gjx.h gjx_scope: one nested `@gen` call of a plan (the range of the flat site table it produced)."""

    _fields_ = [("parent", C.c_int32), ("begin", C.c_int32), ("end", C.c_int32)]


MAX_SCOPES = 16


class LseOut(C.Structure):
    """gjx_lse_out: where a fused importance launch leaves the pass's log-sum-exp."""

    _fields_ = [("e", C.c_void_p), ("q", C.c_void_p), ("lse", C.c_void_p), ("record", C.c_void_p),
                ("tickets", C.c_void_p), ("lse_shifted", C.c_void_p), ("shift", C.c_float)]


LSE_TICKET_WORDS = 17 * 64  # include/gjx.h: GJX_LSE_TICKET_WORDS


class EstimateIO(C.Structure):
    """include/gjx.h gjx_estimate_io: what one gjx_importance_estimate call reads besides the key."""

    _fields_ = [("plan", C.c_void_p), ("n", C.c_uint64), ("input_cols", C.c_void_p), ("n_input_cols", C.c_int32), ("impl", C.c_int32),
                ("row_e", C.c_void_p), ("row_s", C.c_void_p), ("lse", LseOut)]


def key_words(impl: int) -> int:
    """Words per materialised key (gjx.h: GJX_KEY_WORDS): threefry 2, philox 4 (cipher key + lane)."""
    return 4 if impl == RNG_PHILOX else 2


class F32(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("scalar", C.c_float)]


class Arg(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("ref", C.c_int32),
        ("scale", C.c_float),
        ("offset", C.c_float),
        ("table", C.c_void_p),
    ]


class ExprOp(C.Structure):
    _fields_ = [("op", C.c_int32), ("ref", C.c_int32), ("value", C.c_float)]


def expr_arg(prog, keep: list) -> Arg:
    """`prog`: [(opcode, ref, value)] -> a GJX_ARG_EXPR argument.  The ctypes array goes into `keep` (the library copies
    the program at plan creation; until then the caller keeps it alive)."""
    arr = (ExprOp * len(prog))(*[ExprOp(int(o), int(r), float(v)) for o, r, v in prog])
    keep.append(arr)
    return Arg(ARG_EXPR, len(prog), 0.0, 0.0, C.addressof(arr))


class Site(C.Structure):
    _fields_ = [
        ("dist", C.c_int32),
        ("observed", C.c_int32),
        ("out_col", C.c_int32),
        ("n_cat", C.c_int32),
        ("n_rows", C.c_int32),
        ("cat_mode", C.c_int32),
        ("arg", Arg * 2),
        ("obs", Arg),
        ("logits", C.c_void_p),
    ]


class SmcModel(C.Structure):
    _fields_ = [
        ("init_sites", C.POINTER(Site)),
        ("n_init_sites", C.c_int32),
        ("step_sites", C.POINTER(Site)),
        ("n_step_sites", C.c_int32),
        ("init_state", Arg * 4),
        ("next_state", Arg * 4),
        ("n_state", C.c_int32),
        ("n_obs", C.c_int32),
    ]


class ScanModel(C.Structure):
    _fields_ = [
        ("step_sites", C.POINTER(Site)),
        ("n_step_sites", C.c_int32),
        ("next_state", Arg * 4),
        ("n_state", C.c_int32),
        ("n_obs", C.c_int32),
    ]


class ScanIO(C.Structure):
    _fields_ = [
        ("particle_keys", C.c_void_p),
        ("n", C.c_uint64),
        ("n_steps", C.c_int32),
        ("obs", C.c_void_p),
        ("carry0", C.c_void_p),
        ("carry0_cols", C.c_void_p),
        ("value_cols", C.c_void_p),
        ("n_value_cols", C.c_int32),
        ("col_stride", C.c_uint64),
        ("carry_out", C.c_void_p),
        ("score", C.c_void_p),
        ("logw", C.c_void_p),
        ("max_partials", C.c_void_p),
        ("row_e", C.c_void_p),
        ("row_s", C.c_void_p),
        ("lse", C.c_void_p),
    ]


class TileRec(C.Structure):
    """gjx_tile_rec: a tile's mass relative to its own power-of-two anchor."""
    _fields_ = [("s", C.c_uint64), ("e", C.c_int32), ("pad", C.c_int32)]


TILE_REC_WORDS, TILE_SUB_WORDS, TILE_ESS_WORDS = 2, 16, 2  # gjx_tile_rec / gjx_tile_sub / gjx_tile_ess as int64 words
TILE_FRAC = 30  # gjx.h: GJX_TILE_FRAC
TILE_EMPTY = -(1 << 30)


class SmcPop(C.Structure):
    """gjx_smc_pop: a population between two steps."""
    _fields_ = [
        ("state", C.c_void_p * 4),
        ("qw", C.c_void_p),
        ("logw", C.c_void_p),
        ("recs", C.c_void_p),
        ("subs", C.c_void_p),
        ("ess", C.c_void_p),
        ("prefix", C.c_void_p),
    ]


class ShardedIO(C.Structure):
    _fields_ = [
        ("pop", SmcPop * 2),
        ("out_e", C.c_void_p),
        ("out_q", C.c_void_p),
        ("ancestors", C.c_void_p),
        ("ranges", C.c_void_p),
        ("shuffle", C.c_int32),
        ("received", C.POINTER(C.c_uint64)),
        ("stage", C.c_void_p),            # r04: dev [world, tiles_local, 32 B]: adaptive filters on a collective transport
    ]


class Seg(C.Structure):
    """gjx_seg: elements [a, b) of a global column travel to / from `peer`."""
    _fields_ = [("peer", C.c_int32), ("a", C.c_uint64), ("b", C.c_uint64)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int32,
                          C.POINTER(Seg), C.c_int32, C.POINTER(Seg), C.c_int32, C.c_void_p)
STREAM_SYNC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)


COMM_ID_BYTES = 128


class Lgssm(C.Structure):
    _fields_ = [
        ("x0_loc", C.c_float),
        ("x0_scale", C.c_float),
        ("a", C.c_float),
        ("q", C.c_float),
        ("r", C.c_float),
    ]


class Hmm(C.Structure):
    _fields_ = [
        ("n_states", C.c_int32),
        ("init_state", C.c_int32),
        ("trans_logits", C.c_void_p),
        ("obs_logits", C.c_void_p),
    ]


MAX_PEERS = 8


class SmcPeers(C.Structure):
    """gjx_smc_peers: the peer transport of a sharded filter (arenas of identical layout; delta[o] = byte distance from this
    rank's arena to rank o's as mapped in this process; flags / error inside the arena)."""
    _fields_ = [
        ("world", C.c_int32),
        ("rank", C.c_int32),
        ("delta", C.c_int64 * MAX_PEERS),
        ("flags", C.c_void_p),
        ("error", C.c_void_p),
        ("wait_value", C.c_uint64),
        ("timeout_ms", C.c_uint32),
        ("pad", C.c_int32),
        ("signal_recs", C.c_void_p),      # a deferred signal (gjx.h): set by the sharded drivers
        ("signal_ess", C.c_void_p),
        ("signal_first_tile", C.c_uint64),
        ("signal_n_tiles", C.c_uint64),
        ("signal_value", C.c_uint64),
    ]


class SmcConfig(C.Structure):
    _fields_ = [
        ("impl", C.c_int32),
        ("n_total", C.c_uint64),
        ("first_slot", C.c_uint64),
        ("n_local", C.c_uint64),
        ("n_steps", C.c_int32),
        ("step_keys", C.c_void_p),
        ("resample_keys", C.c_void_p),
        ("n_filters", C.c_int32),
        ("filter_stride", C.c_uint64),
        ("ess_threshold", C.c_float),     # 0 / >= 1: resample at every step; (0, 1): only when ESS < threshold * N
        ("resampled_out", C.c_void_p),    # dev int32[T] / [F, T]: 1 where a step began with a resampling
        ("peers", C.POINTER(SmcPeers)),   # r04, nullable: the source population lives in the peers' arenas
    ]


_P = C.c_void_p
_KP = C.POINTER(Keys)

# name -> (restype, argtypes).  Every symbol include/gjx.h declares must be listed here;
# tests/test_abi_symbols.py cross-checks the header against this table and the built .so.
PROTOTYPES = {
    "gjx_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_backend_name": (C.c_char_p, []),
    "gjx_rng_keys": (C.c_int, [_KP, C.c_uint64, _P, _P]),
    "gjx_rng_split_each": (C.c_int, [_KP, C.c_uint64, C.c_uint32, _P, _P]),
    "gjx_rng_bits": (C.c_int, [_KP, C.c_uint32, C.c_uint64, _P, _P]),
    "gjx_sample_logpdf_normal": (C.c_int, [_KP, F32, F32, _P, _P, C.c_uint64, _P]),
    "gjx_sample_logpdf_gamma": (C.c_int, [_KP, F32, F32, _P, _P, C.c_uint64, _P]),
    "gjx_sample_logpdf_beta": (C.c_int, [_KP, F32, F32, _P, _P, C.c_uint64, _P]),
    "gjx_sample_logpdf_bernoulli": (C.c_int, [_KP, F32, _P, _P, C.c_uint64, _P]),
    "gjx_sample_logpdf_categorical": (
        C.c_int,
        [_KP, _P, C.c_uint64, C.c_uint32, _P, C.c_int, _P, _P, C.c_uint64, _P],
    ),
    "gjx_map_f32": (C.c_int, [C.c_int, _P, C.c_float, _P, C.c_uint64, _P]),
    "gjx_logpdf_normal": (C.c_int, [F32, F32, F32, _P, C.c_uint64, _P]),
    "gjx_logpdf_gamma": (C.c_int, [F32, F32, F32, _P, C.c_uint64, _P]),
    "gjx_logpdf_beta": (C.c_int, [F32, F32, F32, _P, C.c_uint64, _P]),
    "gjx_logpdf_bernoulli": (C.c_int, [_P, C.c_int, F32, _P, C.c_uint64, _P]),
    "gjx_logpdf_categorical": (
        C.c_int,
        [_P, C.c_int, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_uint64, _P],
    ),
    "gjx_plan_create": (C.c_int, [C.POINTER(Site), C.c_int, C.POINTER(_P)]),
    "gjx_plan_create_ex": (C.c_int, [C.POINTER(Site), C.c_int, C.c_uint32, C.POINTER(_P)]),
    "gjx_plan_create_scoped": (C.c_int, [C.POINTER(Site), C.c_int, C.POINTER(Scope), C.c_int, C.c_uint32, C.POINTER(_P)]),
    "gjx_plan_destroy": (C.c_int, [_P]),
    "gjx_plan_set_params": (C.c_int, [_P, _P, C.c_int]),
    "gjx_plan_specialized_source": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_plan_compile_check": (C.c_int, [_P, C.c_int]),
    "gjx_plan_prepare": (C.c_int, [_P, _KP]),
    "gjx_jit_stats": (C.c_int, [_P, _P, _P]),
    "gjx_jit_routes": (C.c_int, [_P, _P, _P, _P]),
    "gjx_smc_run_graph_stats": (C.c_int, [_P, _P]),
    "gjx_jit_compile_source": (C.c_int, [C.c_char_p]),
    "gjx_importance_run": (
        C.c_int,
        [_P, _KP, C.POINTER(_P), C.c_int, C.POINTER(_P), C.c_int, _P, _P, C.c_uint64, _P, _P, _P, _P, _P],
    ),
    "gjx_importance_estimate": (C.c_int, [C.POINTER(EstimateIO), C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_float, C.c_void_p]),
    "gjx_importance_run_batch": (
        C.c_int,
        [_P, _KP, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(_P), C.c_int, C.POINTER(_P), C.c_int, _P, _P, C.c_uint64,
         _P, _P, _P, _P],
    ),
    "gjx_workspace_bytes": (C.c_size_t, [C.c_int, C.c_uint64]),
    "gjx_frac_bits": (C.c_int, [C.c_uint64]),
    "gjx_num_tiles": (C.c_uint64, [C.c_uint64]),
    "gjx_num_max_partials": (C.c_uint64, [C.c_uint64]),
    "gjx_row_stats": (C.c_int, [_P, C.c_uint64, _P, _P, _P]),
    "gjx_lse_rows": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, _P, _P]),
    "gjx_lse_rows_batch": (C.c_int, [_P, _P, C.c_uint64, C.c_int32, C.c_uint64, _P, _P, _P, _P, _P]),
    "gjx_lse_combine": (C.c_int, [_P, C.c_int32, C.c_uint64, C.c_int32, C.c_uint64, _P, _P, _P, _P, _P]),
    "gjx_max_f32": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.c_size_t, _P]),
    "gjx_expsum_fix": (C.c_int, [_P, C.c_uint64, _P, C.c_int, _P, _P, C.c_size_t, _P]),
    "gjx_lse_finish": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "gjx_logsumexp_f32": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "gjx_categorical_index": (C.c_int, [_KP, _P, C.c_uint64, _P, C.c_int, _P, C.c_size_t, _P]),
    "gjx_resample_systematic": (
        C.c_int,
        [_KP, _P, C.c_uint64, C.c_uint64, _P, _P, _P, _P, C.c_size_t, _P],
    ),
    "gjx_resample_multinomial": (
        C.c_int,
        [_KP, _P, C.c_uint64, C.c_uint64, _P, _P, _P, _P, C.c_size_t, _P],
    ),
    "gjx_gather_cols": (C.c_int, [_P, C.c_uint64, C.POINTER(_P), C.POINTER(_P), C.c_int, _P]),
    "gjx_smc_tile": (C.c_uint64, []),
    "gjx_smc_run_lgssm": (
        C.c_int,
        [C.POINTER(SmcConfig), C.POINTER(Lgssm), _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P],
    ),
    "gjx_smc_run_hmm": (
        C.c_int,
        [C.POINTER(SmcConfig), C.POINTER(Hmm), _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P],
    ),
    "gjx_smc_plan_create": (C.c_int, [C.POINTER(SmcModel), C.POINTER(_P)]),
    "gjx_smc_plan_create_scoped": (C.c_int, [C.POINTER(SmcModel), C.POINTER(Scope), C.c_int, C.POINTER(Scope), C.c_int, C.POINTER(_P)]),
    "gjx_smc_plan_destroy": (C.c_int, [_P]),
    "gjx_smc_plan_compile_check": (C.c_int, [_P, C.c_int]),
    "gjx_scan_plan_create": (C.c_int, [C.POINTER(ScanModel), C.c_uint32, C.POINTER(_P)]),
    "gjx_scan_plan_create_scoped": (C.c_int, [C.POINTER(ScanModel), C.POINTER(Scope), C.c_int, C.c_uint32, C.POINTER(_P)]),
    "gjx_scan_plan_destroy": (C.c_int, [_P]),
    "gjx_scan_plan_compile_check": (C.c_int, [_P, C.c_int]),
    "gjx_scan_run": (C.c_int, [_P, C.POINTER(ScanIO), _P]),
    "gjx_comm_unique_id": (C.c_int, [_P]),
    "gjx_comm_init_rccl": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "gjx_comm_group_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "gjx_comm_group_destroy": (C.c_int, [_P]),
    "gjx_comm_init_local": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
    "gjx_comm_destroy": (C.c_int, [_P]),
    "gjx_comm_rank": (C.c_int, [_P]),
    "gjx_comm_world": (C.c_int, [_P]),
    "gjx_comm_lse_combine": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    "gjx_smc_sharded_run_lgssm": (C.c_int, [_P, C.POINTER(SmcConfig), C.POINTER(Lgssm), _P, C.POINTER(ShardedIO), _P]),
    "gjx_smc_sharded_run_hmm": (C.c_int, [_P, C.POINTER(SmcConfig), C.POINTER(Hmm), _P, _P, _P, C.POINTER(ShardedIO), _P]),
    "gjx_smc_sharded_run_plan": (C.c_int, [_P, C.POINTER(SmcConfig), _P, _P, C.POINTER(ShardedIO), _P]),
    "gjx_smc_run_plan": (
        C.c_int,
        [C.POINTER(SmcConfig), _P, _P, _P, _P, C.POINTER(_P), _P, _P, _P, C.c_size_t, _P],
    ),
    "gjx_smc_lgssm_step": (
        C.c_int,
        [C.POINTER(SmcConfig), C.POINTER(Lgssm), C.c_int, C.c_float, C.POINTER(SmcPop), C.POINTER(SmcPop), _P, _P, _P, _P],
    ),
    "gjx_smc_hmm_step": (
        C.c_int,
        [C.POINTER(SmcConfig), C.POINTER(Hmm), C.c_int, C.c_int32, C.POINTER(SmcPop), C.POINTER(SmcPop), _P, _P, _P, _P, _P, _P],
    ),
    "gjx_smc_plan_step": (C.c_int, [C.POINTER(SmcConfig), _P, C.c_int, _P, C.POINTER(SmcPop), C.POINTER(SmcPop), _P, _P, _P, _P]),
    "gjx_smc_finish": (C.c_int, [C.POINTER(SmcConfig), _P, _P, _P, _P]),
    "gjx_smc_source_ranges": (C.c_int, [C.POINTER(SmcConfig), _P, _P, C.c_int, C.c_int64, _P, _P]),
    "gjx_tile_weights": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P]),
    "gjx_tile_merge": (C.c_int, [_P, C.c_uint64, _P, _P, _P]),
    "gjx_comm_init_callbacks": (C.c_int, [C.c_int, C.c_int, ALLGATHER_FN, EXCHANGE_FN, STREAM_SYNC_FN, _P, C.POINTER(_P)]),
    "gjx_categorical_index_batch": (C.c_int, [_KP, C.c_int32, _P, C.c_uint64, C.c_uint64, _P, _P]),
    "gjx_comm_init_peers": (C.c_int, [C.POINTER(SmcPeers), _P, C.c_int, C.POINTER(_P)]),
    "gjx_smc_peer_signal": (C.c_int, [C.POINTER(SmcPeers), _P, _P, C.c_uint64, C.c_uint64, C.c_uint64, _P]),
    "gjx_smc_peer_wait": (C.c_int, [C.POINTER(SmcPeers), C.c_uint64, _P]),
    "gjx_smc_peer_signal_fused": (C.c_int, [C.POINTER(SmcConfig)]),
    "gjx_smc_records_pack": (C.c_int, [C.POINTER(SmcConfig), C.c_int, C.c_int, _P, _P, _P, _P]),
    "gjx_hmm_alias_words": (C.c_uint64, [C.c_int32]),
    "gjx_hmm_prepare": (C.c_int, [C.POINTER(Hmm), _P, _P, _P]),
}

class PathsIO(C.Structure):
    """gjx_paths_io (include/gjx_paths.h): a trajectory trace-back over a recorded filter history."""
    _fields_ = [
        ("n_steps", C.c_int32),
        ("n_cols", C.c_int32),
        ("n", C.c_uint64),
        ("m", C.c_uint64),
        ("ancestors", C.c_void_p),
        ("anc_stride", C.c_uint64),
        ("leaves", C.c_void_p),
        ("cols", C.c_void_p * PATHS_MAX_COLS),
        ("col_stride", C.c_uint64 * PATHS_MAX_COLS),
        ("col_is_f32", C.c_int32 * PATHS_MAX_COLS),
        ("lineage_out", C.c_void_p),
        ("lineage_stride", C.c_uint64),
        ("paths_out", C.c_void_p * PATHS_MAX_COLS),
        ("paths_stride", C.c_uint64 * PATHS_MAX_COLS),
        ("sum_out", C.c_void_p),
        ("sumsq_out", C.c_void_p),
        ("unique_out", C.c_void_p),
        ("ticket", C.c_void_p),
        ("flags", C.c_uint32),
        ("max_workgroups", C.c_uint32),
    ]


# include/gjx_paths.h: a SECOND header with a version of its own — exported by libgjx_hip.so only and bound if present
# (GjxLib); PROTOTYPES above stays exactly the symbol set of gjx.h, which the CPU oracle restates.
PATHS_PROTOTYPES = {
    "gjx_paths_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_paths_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_uint64, C.c_int32]),
    "gjx_paths_trace": (C.c_int, [C.POINTER(PathsIO), _P, C.c_size_t, _P]),
}
PATHS_ABI_VERSION = (0, 1)

# include/gjx_guided.h: a THIRD header, same arrangement — guided particle filters (proposed / guided site modes)
SITE_PROPOSED, SITE_GUIDED = 2, 3  # gjx_guided.h: GJX_SITE_PROPOSED / GJX_SITE_GUIDED (values of Site.observed)
GUIDED_PROTOTYPES = {
    "gjx_guided_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_smc_plan_create_guided": (C.c_int, [C.POINTER(SmcModel), C.POINTER(_P)]),
    "gjx_smc_plan_source": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
}
GUIDED_ABI_VERSION = (0, 1)

# include/gjx_backsim.h: a FOURTH header, same arrangement — backward-simulation smoothing over a recorded history
ARG_NEXT = 8  # gjx_backsim.h: GJX_ARG_NEXT (Arg.kind, in Site.obs of a transition table)


class BacksimIO(C.Structure):
    """gjx_backsim_io (include/gjx_backsim.h)."""
    _fields_ = [
        ("n_steps", C.c_int32),
        ("impl", C.c_int32),
        ("n", C.c_uint64),
        ("m", C.c_uint64),
        ("key", C.c_uint32 * 2),
        ("key_lane", C.c_uint64),
        ("cols", C.c_void_p * SMC_MAX_STATE),
        ("col_stride", C.c_uint64 * SMC_MAX_STATE),
        ("col_is_i32", C.c_int32 * SMC_MAX_STATE),
        ("logw", C.c_void_p),
        ("logw_stride", C.c_uint64),
        ("obs", C.c_void_p),
        ("lineage_out", C.c_void_p),
        ("lineage_stride", C.c_uint64),
        ("paths_out", C.c_void_p * SMC_MAX_STATE),
        ("paths_stride", C.c_uint64 * SMC_MAX_STATE),
        ("max_workgroups", C.c_uint32),
    ]


BACKSIM_PROTOTYPES = {
    "gjx_backsim_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_backsim_plan_create": (C.c_int, [C.POINTER(Site), C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(_P)]),
    "gjx_backsim_plan_destroy": (C.c_int, [_P]),
    "gjx_backsim_plan_source": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_backsim_plan_compile_check": (C.c_int, [_P, C.c_int]),
    "gjx_backsim_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_uint64]),
    "gjx_backsim_run": (C.c_int, [_P, C.POINTER(BacksimIO), _P, C.c_size_t, _P]),
}
BACKSIM_ABI_VERSION = (0, 1)


# include/gjx_backmove.h: a FIFTH header, same arrangement — MCMC backward simulation (K Metropolis-Hastings moves per path
# and step, cost independent of n) on an existing gjx_backsim_plan
class BackmoveIO(C.Structure):
    """gjx_backmove_io (include/gjx_backmove.h): the fields of gjx_backsim_io, then ancestors / anc_stride / n_moves."""
    _fields_ = BacksimIO._fields_ + [
        ("ancestors", C.c_void_p),
        ("anc_stride", C.c_uint64),
        ("n_moves", C.c_int32),
    ]


BACKMOVE_PROTOTYPES = {
    "gjx_backmove_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_backmove_plan_source": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_backmove_plan_compile_check": (C.c_int, [_P, C.c_int]),
    "gjx_backmove_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_uint64, C.c_uint64]),
    "gjx_backmove_run": (C.c_int, [_P, C.POINTER(BackmoveIO), _P, C.c_size_t, _P]),
}
BACKMOVE_ABI_VERSION = (0, 1)
BACKMOVE_MAX_MOVES = 256  # gjx_backmove.h: GJX_BACKMOVE_MAX_MOVES

# include/gjx_smc_params.h: a SIXTH header, same arrangement — parameterised state-space models (one parameter row per
# filter of a launch) as plain gjx_smc_plan objects
SMC_PARAMS_PROTOTYPES = {
    "gjx_smc_params_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_smc_plan_create_params": (C.c_int, [C.POINTER(SmcModel), C.POINTER(Scope), C.c_int, C.POINTER(Scope), C.c_int, C.c_int,
                                             C.POINTER(_P)]),
    "gjx_smc_plan_set_params": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
}
SMC_PARAMS_ABI_VERSION = (0, 1)
SMC_PARAMS_MAX_ROWS = 16  # gjx_smc_params.h: GJX_SMC_PARAMS_MAX_ROWS

# include/gjx_csmc.h: a SEVENTH header, same arrangement — the conditional step (slot n - 1 retained) of a gjx_smc_plan
class CsmcPath(C.Structure):
    """gjx_csmc_path (include/gjx_csmc.h): one device f32[T] per state component."""
    _fields_ = [("path", C.c_void_p * SMC_MAX_STATE)]


CSMC_PROTOTYPES = {
    "gjx_csmc_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_smc_plan_step_conditional": (C.c_int, [C.POINTER(SmcConfig), _P, C.c_int, _P, C.POINTER(SmcPop), C.POINTER(SmcPop), _P, _P, _P,
                                                C.POINTER(CsmcPath), _P]),
    "gjx_csmc_plan_source": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_csmc_plan_compile_check": (C.c_int, [_P, C.c_int]),
}
CSMC_ABI_VERSION = (0, 1)

# include/gjx_temper.h: an EIGHTH header, same arrangement — tempered SMC for static models: a plan kind of its own over a
# flat importance-style site table, the fused resample-move launch and the one-launch ESS ladder
TEMPER_MAX_LATENTS = 16  # gjx_temper.h: GJX_TEMPER_MAX_LATENTS
TEMPER_MAX_MOVES = 256   # ... GJX_TEMPER_MAX_MOVES
TEMPER_MAX_LADDER = 64   # ... GJX_TEMPER_MAX_LADDER


class TemperIO(C.Structure):
    """gjx_temper_io (include/gjx_temper.h)."""
    _fields_ = [
        ("impl", C.c_int32),
        ("n_moves", C.c_int32),
        ("recompute", C.c_int32),
        ("beta", C.c_float),
        ("n", C.c_uint64),
        ("key", C.c_uint32 * 2),
        ("key_lane", C.c_uint64),
        ("x_in", C.c_void_p * TEMPER_MAX_LATENTS),
        ("lp_in", C.c_void_p),
        ("ll_in", C.c_void_p),
        ("ancestors", C.c_void_p),
        ("scales", C.POINTER(C.c_float)),
        ("input_cols", C.POINTER(C.c_void_p)),
        ("n_input_cols", C.c_int32),
        ("x_out", C.c_void_p * TEMPER_MAX_LATENTS),
        ("lp_out", C.c_void_p),
        ("ll_out", C.c_void_p),
        ("n_accept", C.c_void_p),
        ("max_workgroups", C.c_uint32),
    ]


TEMPER_PROTOTYPES = {
    "gjx_temper_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_temper_plan_create": (C.c_int, [C.POINTER(Site), C.c_int, C.c_uint32, C.POINTER(_P)]),
    "gjx_temper_plan_destroy": (C.c_int, [_P]),
    "gjx_temper_plan_set_params": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "gjx_temper_plan_n_latents": (C.c_int, [_P]),
    "gjx_temper_plan_source": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_temper_plan_compile_check": (C.c_int, [_P, C.c_int]),
    "gjx_temper_move": (C.c_int, [_P, C.POINTER(TemperIO), _P]),
    "gjx_temper_ladder_blocks": (C.c_uint32, [C.c_uint64]),
    "gjx_temper_ladder_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_int32]),
    "gjx_temper_ess_ladder": (C.c_int, [_P, C.c_uint64, C.POINTER(C.c_float), C.c_int32, _P, _P, C.c_size_t, _P]),
}
TEMPER_ABI_VERSION = (0, 1)

# include/gjx_plate.h: a NINTH header, same arrangement — plated likelihoods of a tempered plan: one observed site looped over
# the rows of device data columns (a site mode, an argument kind and a program leaf of its own, a creator and a setter)
SITE_PLATED = 4          # gjx_plate.h: GJX_SITE_PLATED (gjx_site.observed)
ARG_DATA = 9             # ... GJX_ARG_DATA (gjx_arg.kind; GJX_ARG_NEXT is 8)
EXPR_DATA = 21           # ... GJX_EXPR_DATA (gjx_expr_op.op)
PLATE_MAX_COLS = 16      # ... GJX_PLATE_MAX_COLS
PLATE_PROTOTYPES = {
    "gjx_plate_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_temper_plan_create_plated": (C.c_int, [C.POINTER(Site), C.c_int, C.c_uint32, C.POINTER(_P)]),
    "gjx_temper_plan_set_data": (C.c_int, [_P, C.POINTER(C.c_void_p), C.c_int, C.c_uint64]),
}
PLATE_ABI_VERSION = (0, 1)

# include/gjx_pointwise.h: a TENTH header, same arrangement — the per-row log-likelihood table of a plated tempered plan reduced
# over the particles (log-sum-exp, two moments, count): what lppd, WAIC and held-out scores are made of
class PointwiseIO(C.Structure):
    """gjx_pointwise_io (include/gjx_pointwise.h)."""
    _fields_ = [
        ("n", C.c_uint64),
        ("x", C.c_void_p * TEMPER_MAX_LATENTS),
        ("out", C.c_void_p),
        ("ws", C.c_void_p),
        ("ws_bytes", C.c_size_t),
    ]


POINTWISE_PROTOTYPES = {
    "gjx_pointwise_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_pointwise_chunks": (C.c_uint32, [C.c_uint64, C.c_uint64]),
    "gjx_pointwise_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_uint64]),
    "gjx_temper_pointwise": (C.c_int, [_P, C.POINTER(PointwiseIO), _P]),
    "gjx_pointwise_source": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_pointwise_compile_check": (C.c_int, [_P]),
}
POINTWISE_ABI_VERSION = (0, 1)

# include/gjx_psis.h: a THIRTEENTH header, same arrangement — Pareto-smoothed importance-sampling leave-one-out over the same
# table: per row the M + 1 smallest entries over the particles selected exactly, the generalised-Pareto fit of that tail, its
# shape k-hat and elpd_loo.  It builds on gjx_plate.h alone and is bound right before it (the suites of the later headers pin the
# end of PLAN_HEADERS).
PSIS_MAX_TAIL = 4095     # gjx_psis.h: GJX_PSIS_MAX_TAIL


class PsisIO(C.Structure):
    """gjx_psis_io (include/gjx_psis.h)."""
    _fields_ = [
        ("n", C.c_uint64),
        ("x", C.c_void_p * TEMPER_MAX_LATENTS),
        ("tail_len", C.c_uint32),
        ("out", C.c_void_p),
        ("tail", C.c_void_p),
        ("ws", C.c_void_p),
        ("ws_bytes", C.c_size_t),
    ]


PSIS_PROTOTYPES = {
    "gjx_psis_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_psis_tail_len": (C.c_uint32, [C.c_uint64, C.c_double]),
    "gjx_psis_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_uint64, C.c_uint32]),
    "gjx_temper_psis": (C.c_int, [_P, C.POINTER(PsisIO), _P]),
    "gjx_psis_source": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_psis_compile_check": (C.c_int, [_P]),
}
PSIS_ABI_VERSION = (0, 1)

# include/gjx_predictive.h: a TWELFTH header, same arrangement — posterior predictive draws of a plated tempered plan: per row
# and plated site the moments of the replicated data over the particles, its position against the observed value, and a
# strided subset of the draws themselves.  It builds on gjx_plate.h alone and is bound right after it.
class PredictiveIO(C.Structure):
    """gjx_predictive_io (include/gjx_predictive.h)."""
    _fields_ = [
        ("n", C.c_uint64),
        ("x", C.c_void_p * TEMPER_MAX_LATENTS),
        ("out", C.c_void_p),
        ("draws", C.c_void_p),
        ("draw_stride", C.c_uint64),
        ("ws", C.c_void_p),
        ("ws_bytes", C.c_size_t),
    ]


PREDICTIVE_PROTOTYPES = {
    "gjx_predictive_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_predictive_chunks": (C.c_uint32, [C.c_uint64, C.c_uint64]),
    "gjx_predictive_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_uint64, C.c_int32]),
    "gjx_temper_predictive": (C.c_int, [_P, C.POINTER(Keys), C.POINTER(PredictiveIO), _P]),
    "gjx_predictive_source": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_predictive_compile_check": (C.c_int, [_P, C.c_int]),
}
PREDICTIVE_ABI_VERSION = (0, 1)

# include/gjx_temper_cov.h: an ELEVENTH header, same arrangement — full-covariance proposals for the tempered move: the one-launch
# weighted moments of a population with the proposal factor built on the device, and the move through that factor
class TemperMomentsIO(C.Structure):
    """gjx_temper_moments_io (include/gjx_temper_cov.h)."""
    _fields_ = [
        ("n", C.c_uint64),
        ("n_latents", C.c_int32),
        ("x", C.c_void_p * TEMPER_MAX_LATENTS),
        ("lw", C.c_void_p),
        ("moments", C.c_void_p),
        ("factor", C.c_void_p),
        ("scales", C.c_void_p),
        ("n_degenerate", C.c_void_p),
        ("ws", C.c_void_p),
        ("ws_bytes", C.c_size_t),
        ("max_workgroups", C.c_uint32),
    ]


TEMPER_COV_PROTOTYPES = {
    "gjx_temper_cov_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_temper_moments_workspace_bytes": (C.c_size_t, [C.c_uint64, C.c_int32]),
    "gjx_temper_moments": (C.c_int, [C.POINTER(TemperMomentsIO), _P]),
    "gjx_temper_move_cov": (C.c_int, [_P, C.POINTER(TemperIO), _P, _P]),
    "gjx_temper_cov_source": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_temper_cov_compile_check": (C.c_int, [_P, C.c_int]),
}
TEMPER_COV_ABI_VERSION = (0, 1)

# include/gjx_counts.h: a FOURTEENTH header, same arrangement — the count families Poisson and NegativeBinomial: two
# distribution ids, their stand-alone density and draw kernels, and the tempered creator that accepts them at observed and
# plated sites.  Bound between "temper" and "psis": the one slot that keeps what the suites of the other headers pin.
DIST_POISSON = 5             # gjx_counts.h: GJX_DIST_POISSON (a0 = rate)
DIST_NEGATIVE_BINOMIAL = 6   # ... GJX_DIST_NEGATIVE_BINOMIAL (a0 = total_count, a1 = probs)
COUNT_DISTS = (DIST_POISSON, DIST_NEGATIVE_BINOMIAL)
COUNTS_MAX_OBSERVED = 1 << 24  # ... GJX_COUNTS_MAX_OBSERVED
COUNTS_PROTOTYPES = {
    "gjx_counts_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_logpdf_poisson": (C.c_int, [_P, C.c_int, F32, _P, C.c_uint64, _P]),
    "gjx_logpdf_negative_binomial": (C.c_int, [_P, C.c_int, F32, F32, _P, C.c_uint64, _P]),
    "gjx_sample_logpdf_poisson": (C.c_int, [_KP, F32, _P, _P, C.c_uint64, _P]),
    "gjx_sample_logpdf_negative_binomial": (C.c_int, [_KP, F32, F32, _P, _P, C.c_uint64, _P]),
    "gjx_temper_plan_create_counts": (C.c_int, [C.POINTER(Site), C.c_int, C.c_uint32, C.POINTER(_P)]),
}
COUNTS_ABI_VERSION = (0, 1)

# include/gjx_group.h: a FIFTEENTH header, same arrangement — grouped latents of a tempered plan: a site mode, an argument kind
# and a program leaf of its own, a creator, the setter of the group offsets and the grouped move.  Bound before "temper": the
# slots after it are pinned by the suites of the other headers.
SITE_GROUPED = 5          # gjx_group.h: GJX_SITE_GROUPED (gjx_site.observed)
ARG_GROUP = 10            # ... GJX_ARG_GROUP (gjx_arg.kind)
EXPR_GROUP = 22           # ... GJX_EXPR_GROUP (gjx_expr_op.op)
GROUP_MAX_SITES = 4       # ... GJX_GROUP_MAX_SITES
GROUP_MAX_GROUPS = 1 << 24  # ... GJX_GROUP_MAX_GROUPS


class GroupIO(C.Structure):
    """gjx_group_io (include/gjx_group.h)."""
    _fields_ = [
        ("t", TemperIO),
        ("z_in", C.c_void_p * GROUP_MAX_SITES),
        ("z_out", C.c_void_p * GROUP_MAX_SITES),
        ("z_scales", C.c_void_p * GROUP_MAX_SITES),
        ("n_accept_z", C.c_void_p),
        ("init", C.c_int32),
        ("init_key", C.c_uint32 * 2),
        ("init_key_lane", C.c_uint64),
    ]


GROUP_PROTOTYPES = {
    "gjx_group_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_temper_plan_create_grouped": (C.c_int, [C.POINTER(Site), C.c_int, C.c_uint32, C.POINTER(_P)]),
    "gjx_temper_plan_set_groups": (C.c_int, [_P, _P, C.c_uint32]),
    "gjx_temper_plan_n_grouped": (C.c_int, [_P]),
    "gjx_temper_move_grouped": (C.c_int, [_P, C.POINTER(GroupIO), _P]),
}
GROUP_ABI_VERSION = (0, 1)

# include/gjx_group_checks.h: a SIXTEENTH header, same arrangement — pointwise densities, PSIS-LOO and predictive draws of a
# plan with grouped latents: the io structs of the flat headers plus the grouped columns.  Bound directly after "group".


class GroupCols(C.Structure):
    """gjx_group_cols (include/gjx_group_checks.h)."""
    _fields_ = [("z", C.c_void_p * GROUP_MAX_SITES)]


GROUP_CHECKS_PROTOTYPES = {
    "gjx_group_checks_version": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gjx_temper_pointwise_grouped": (C.c_int, [_P, C.POINTER(PointwiseIO), C.POINTER(GroupCols), _P]),
    "gjx_temper_psis_grouped": (C.c_int, [_P, C.POINTER(PsisIO), C.POINTER(GroupCols), _P]),
    "gjx_temper_predictive_grouped": (C.c_int, [_P, C.POINTER(Keys), C.POINTER(PredictiveIO), C.POINTER(GroupCols), _P]),
    "gjx_group_checks_source": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gjx_group_checks_compile_check": (C.c_int, [_P, C.c_int, C.c_int]),
}
GROUP_CHECKS_ABI_VERSION = (0, 1)

# The optional headers, in the order they are bound: every one is exported by libgjx_hip.so only and bound if present.
class Header(collections.namedtuple("Header", "key header version_fn prototypes version_name unavailable")):
    @property
    def version(self):  # the (major, minor) these bindings are written for: the module constant as it is when a library loads
        return globals()[self.version_name]


OPTIONAL_HEADERS = {h.key: h for h in (
    Header("paths", "gjx_paths.h", "gjx_paths_version", PATHS_PROTOTYPES, "PATHS_ABI_VERSION", PathsUnavailable),
    Header("guided", "gjx_guided.h", "gjx_guided_version", GUIDED_PROTOTYPES, "GUIDED_ABI_VERSION", GuidedUnavailable),
    Header("backsim", "gjx_backsim.h", "gjx_backsim_version", BACKSIM_PROTOTYPES, "BACKSIM_ABI_VERSION", BacksimUnavailable),
)}
# Headers that build on an optional header's objects (gjx_backmove.h works on a gjx_backsim_plan): the same tuples, bound
# after OPTIONAL_HEADERS and looked up with them everywhere.
EXTENSION_HEADERS = {h.key: h for h in (
    Header("backmove", "gjx_backmove.h", "gjx_backmove_version", BACKMOVE_PROTOTYPES, "BACKMOVE_ABI_VERSION", BackmoveUnavailable),
)}
# Headers that add creators / setters for the objects of gjx.h itself (gjx_smc_params.h makes and configures a
# gjx_smc_plan).  A table of its own for the reason EXTENSION_HEADERS is one: the suites of the earlier headers pin the
# contents of the two tables above; bound after them and looked up with them everywhere.
PLAN_HEADERS = {h.key: h for h in (
    Header("smc_params", "gjx_smc_params.h", "gjx_smc_params_version", SMC_PARAMS_PROTOTYPES, "SMC_PARAMS_ABI_VERSION",
           SmcParamsUnavailable),
    Header("csmc", "gjx_csmc.h", "gjx_csmc_version", CSMC_PROTOTYPES, "CSMC_ABI_VERSION", CsmcUnavailable),
    Header("group", "gjx_group.h", "gjx_group_version", GROUP_PROTOTYPES, "GROUP_ABI_VERSION", GroupUnavailable),
    Header("group_checks", "gjx_group_checks.h", "gjx_group_checks_version", GROUP_CHECKS_PROTOTYPES, "GROUP_CHECKS_ABI_VERSION",
           GroupChecksUnavailable),
    Header("temper", "gjx_temper.h", "gjx_temper_version", TEMPER_PROTOTYPES, "TEMPER_ABI_VERSION", TemperUnavailable),
    Header("counts", "gjx_counts.h", "gjx_counts_version", COUNTS_PROTOTYPES, "COUNTS_ABI_VERSION", CountsUnavailable),
    Header("psis", "gjx_psis.h", "gjx_psis_version", PSIS_PROTOTYPES, "PSIS_ABI_VERSION", PsisUnavailable),
    Header("plate", "gjx_plate.h", "gjx_plate_version", PLATE_PROTOTYPES, "PLATE_ABI_VERSION", PlateUnavailable),
    Header("predictive", "gjx_predictive.h", "gjx_predictive_version", PREDICTIVE_PROTOTYPES, "PREDICTIVE_ABI_VERSION",
           PredictiveUnavailable),
    Header("pointwise", "gjx_pointwise.h", "gjx_pointwise_version", POINTWISE_PROTOTYPES, "POINTWISE_ABI_VERSION",
           PointwiseUnavailable),
)}
# Headers that add entry points over the plans of a PLAN_HEADERS header (gjx_temper_cov.h moves a gjx_temper_plan).  A table of
# its own for the same reason again: the suites of the earlier headers pin the contents of the three tables above; bound
# after them and looked up with them everywhere.
MOVE_HEADERS = {h.key: h for h in (
    Header("temper_cov", "gjx_temper_cov.h", "gjx_temper_cov_version", TEMPER_COV_PROTOTYPES, "TEMPER_COV_ABI_VERSION",
           TemperCovUnavailable),
)}


def all_optional_headers():
    """Every header next to gjx.h, in binding order: OPTIONAL_HEADERS, then EXTENSION_HEADERS, then PLAN_HEADERS, then
    MOVE_HEADERS."""
    return (*OPTIONAL_HEADERS.values(), *EXTENSION_HEADERS.values(), *PLAN_HEADERS.values(), *MOVE_HEADERS.values())


_HEADER_OF = {name: h for h in all_optional_headers() for name in h.prototypes}  # entry point -> its optional header

_NO_STATUS = {
    "gjx_temper_plan_n_latents",
    "gjx_temper_plan_n_grouped",
    "gjx_temper_ladder_blocks",
    "gjx_temper_ladder_workspace_bytes",
    "gjx_pointwise_chunks",
    "gjx_pointwise_workspace_bytes",
    "gjx_predictive_chunks",
    "gjx_psis_tail_len",
    "gjx_psis_workspace_bytes",
    "gjx_predictive_workspace_bytes",
    "gjx_temper_moments_workspace_bytes",
    "gjx_backmove_workspace_bytes",
    "gjx_backsim_workspace_bytes",
    "gjx_paths_workspace_bytes",
    "gjx_backend_name",
    "gjx_workspace_bytes",
    "gjx_frac_bits",
    "gjx_smc_tile",
    "gjx_num_tiles",
    "gjx_num_max_partials",
    "gjx_hmm_alias_words",
    "gjx_comm_rank",
    "gjx_comm_world",
    "gjx_smc_peer_signal_fused",
}


# The (major, minor) of include/gjx.h these bindings were written for.  Struct layouts and the sampling spec change behind
# unchanged entry points from minor to minor (0.7 -> 0.8: LseOut / SmcConfig / ShardedIO layouts, the Philox Normal spec), so a
# library of another version is refused at load: with mismatched layouts it would read garbage pointers (silent corruption,
# or a GPU fault on a shared box).
ABI_VERSION = (0, 10)


class AbiVersionMismatch(RuntimeError):
    pass


_CORE_HEADER = Header("core", "gjx.h", "gjx_version", PROTOTYPES, "ABI_VERSION", None)


class GjxLib:
    """A loaded implementation of include/gjx.h.  `device_type` is the torch device type whose
    memory the library's "dev" pointers refer to ("cuda" for libgjx_hip.so)."""

    def __init__(self, path: str, device_type: str):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path = path
        self.device_type = device_type
        self._dll = C.CDLL(path)
        # gjx.h, then every optional header the library has (libgjx_hip.so all of them, the oracle library none).  The version
        # FIRST (gjx_version exists in every build): a library of another minor may lack newer symbols, and the useful error
        # is "wrong version", not "missing symbol"
        self.has = {}
        major, minor = C.c_int(-1), C.c_int(-1)
        for h in (_CORE_HEADER, *all_optional_headers()):
            if h is not _CORE_HEADER:
                self.has[h.key] = hasattr(self._dll, h.version_fn)
                setattr(self, "has_" + h.key, self.has[h.key])
                if not self.has[h.key]:
                    continue
            vfn = getattr(self._dll, h.version_fn)
            vfn.restype, vfn.argtypes = h.prototypes[h.version_fn]
            vfn(C.byref(major), C.byref(minor))
            if (major.value, minor.value) != h.version:
                raise AbiVersionMismatch(
                    f"{path} implements {h.header} {major.value}.{minor.value}; these bindings are written for "
                    f"{h.version[0]}.{h.version[1]}" + (
                        " (struct layouts and the sampling spec differ between minors): rebuild the library from this tree, or "
                        "run the other library with its own tree's bindings" if h is _CORE_HEADER
                        else ": rebuild the library from this tree"))
            for name, (res, args) in h.prototypes.items():
                fn = getattr(self._dll, name)  # AttributeError => ABI symbol missing: fail loudly
                fn.restype = res
                fn.argtypes = args
                setattr(self, "_" + name, fn)
        self.version = _CORE_HEADER.version  # (checked above)
        self.name = self._gjx_backend_name().decode()

    def require(self, key: str, fn_name: str):
        """Raise the header's *Unavailable, naming `fn_name`, on a library without the optional header `key`."""
        if not self.has[key]:
            raise next(h for h in all_optional_headers() if h.key == key).unavailable(fn_name, self.name)

    def call(self, name: str, *args):
        h = _HEADER_OF.get(name)
        if h is not None and not self.has[h.key]:
            raise h.unavailable(name, self.name)
        rc = getattr(self, "_" + name)(*args)
        if name not in _NO_STATUS and rc != GJX_OK:
            raise GjxError(name, rc)
        return rc
