"""ctypes mirror of include/flashvit.h — the host-side Python face of libflashvit.so.

There is deliberately no CPU fallback here: if the HIP library is missing or no GPU is
visible, construction fails loudly.  (The CPU restatement lives in oracle/ and is test
infrastructure; this module never imports it.)
"""
import ctypes
import os

import numpy as np

from . import build as _build

MODE_REFERENCE = 0
MODE_SINGLE_PASS = 1
KERNEL_AUTO, KERNEL_F64_STREAM, KERNEL_F32_REFINE, KERNEL_F16_REFINE, KERNEL_Q16_REFINE, KERNEL_SPARSE_Q16 = 0, 1, 2, 3, 4, 5
KERNEL_U16_REFINE = 6
KERNEL_SPARSE_CSR = 7                  # reported by stats()["kernel"] for a model set by set_model_sparse; never chosen
KERNEL_CSR_F64 = 8                     # models set by set_model_sparse: the float64 walk (entries above 1, emission scores above 0)
OPT_KERNEL, OPT_MAX_BATCH, OPT_PROFILE, OPT_SEL_MARGIN, OPT_DEBUG = 1, 2, 3, 4, 100
OPT_FLAT_GENERATIONS = 5               # 0 off, 1 auto (default), 2 on: all right-hand generations at once from the whole-sequence chain
OPT_ROW_CODES = 6                      # 0 off, 1 auto (default), 2 on: the packed kernel's score codes come from the row's producer
OPT_SPARSE_BEAM = 7                    # 0 (default) / 1: the beam calls run on a model set by set_model_sparse (refused under 0)
FLAT_OFF, FLAT_AUTO, FLAT_ON = 0, 1, 2
DEBUG_TIMING_ONLY = (1 << 0) | (1 << 4) | (1 << 5) | (1 << 11) | (1 << 12)      # refused by the shipped library
DEBUG_BATCH_GEN0_SERIAL = 1 << 28      # decode_full_batch: the whole-sequence passes on one stream (speed only)
DEBUG_BEAM_BATCH_GEN0_OTHER = 1 << 29  # decode_beam_batch: the whole-sequence passes in the launch form that is not the default (speed only)
DEBUG_CSR_ROWS_IN_MEMORY = 1 << 31     # sparse-set models: the step kernel reads its score rows from memory at any K (speed only)
# FV_TV_CSR64_* of include/flashvit_testing.h (test_forward's variants): trellis_step_csr_f64<NB, *> for NB = 1, 2, 4, 8, and the
# bit every launch that read its score rows from memory sets in addition
TV_CSR64_NB = (1 << 58, 1 << 59, 1 << 60, 1 << 61)
TV_CSR64_MEM = 1 << 62
TV_BEAM_CSR = (1 << 46) | (1 << 47)    # FV_TV_BEAM_CSR: test_beam_step ran the CSR scatter + finish (OPT_SPARSE_BEAM); the pair of the W4 / W16 bits
TV_ROW_CODES = 1 << 63                 # a packed-kernel launch copied its score codes from the producers (OPT_ROW_CODES)
WARN_BEAM_MISS = 1
ERR_ARG, ERR_NOMEM, ERR_NO_PRED, ERR_DEVICE, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6
UNIQUE_ID_BYTES = 128
EMIS_LOG_F32, EMIS_LOG_F64 = 0, 1     # dtype of fv_set_emissions
EMIS_LOG_F16, EMIS_LOG_BF16 = 2, 3     # IEEE binary16 / bfloat16 (numpy has no bfloat16: a torch tensor, or a pointer in the tuple form)
_EMIS_OF_NUMPY = {np.dtype(np.float32): EMIS_LOG_F32, np.dtype(np.float64): EMIS_LOG_F64, np.dtype(np.float16): EMIS_LOG_F16}


class Stats(ctypes.Structure):
    _fields_ = [("set_model_ms", ctypes.c_double), ("decode_ms", ctypes.c_double), ("gpu_ms", ctypes.c_double),
                ("top_pass_ms", ctypes.c_double), ("top_steps_ms", ctypes.c_double),
                ("step_kernel_ms", ctypes.c_double),
                ("step_launches", ctypes.c_longlong), ("task_steps", ctypes.c_longlong),
                ("column_steps", ctypes.c_longlong),
                ("cells", ctypes.c_longlong), ("alg_bytes", ctypes.c_longlong),
                ("table_bytes_per_step", ctypes.c_longlong), ("device_bytes", ctypes.c_longlong),
                ("refine_near", ctypes.c_longlong), ("refine_rescan", ctypes.c_longlong),
                ("beam_exact_sets", ctypes.c_longlong), ("beam_ties", ctypes.c_longlong),
                ("beam_dup_cols", ctypes.c_longlong), ("beam_dup_steps", ctypes.c_longlong),
                ("beam_cand_selects", ctypes.c_longlong), ("density", ctypes.c_double),
                ("passes", ctypes.c_int), ("generations", ctypes.c_int), ("kernel", ctypes.c_int),
                ("ranks", ctypes.c_int), ("refine_saturated", ctypes.c_longlong),
                ("beam_spec_steps", ctypes.c_longlong), ("beam_reach_events", ctypes.c_longlong),
                ("beam_list_short", ctypes.c_longlong), ("beam_list_long", ctypes.c_longlong), ("beam_list_entries", ctypes.c_longlong),
                ("beam_chain_cuts", ctypes.c_longlong),
                ("flat_passes", ctypes.c_int), ("flat_missed", ctypes.c_int), ("flat_first_miss", ctypes.c_int),
                ("set_emissions_ms", ctypes.c_double), ("emission_rows", ctypes.c_longlong),
                ("bt_restarts", ctypes.c_longlong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class StreamStats(ctypes.Structure):
    """fv_stream_stats: the open stream, or the last one closed or aborted."""
    _fields_ = [("times", ctypes.c_longlong), ("committed", ctypes.c_longlong), ("pushes", ctypes.c_longlong),
                ("checks", ctypes.c_longlong), ("commits", ctypes.c_longlong), ("lag_max", ctypes.c_longlong),
                ("arg_rows_capacity", ctypes.c_longlong), ("regrows", ctypes.c_longlong), ("bt_restarts", ctypes.c_longlong),
                ("push_ms_total", ctypes.c_double), ("kernel", ctypes.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class StreamsStats(ctypes.Structure):
    """fv_streams_stats: the open set of streams, or the last one ended, summed over its life."""
    _fields_ = [("calls", ctypes.c_longlong), ("step_launches", ctypes.c_longlong), ("task_steps", ctypes.c_longlong),
                ("check_launches", ctypes.c_longlong), ("check_slots", ctypes.c_longlong), ("syncs", ctypes.c_longlong),
                ("nslots", ctypes.c_int), ("batch_cap", ctypes.c_int), ("kernel", ctypes.c_int), ("push_ms_total", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LagStats(ctypes.Structure):
    """fv_lag_stats: the forced commits of a lag-bounded stream or slot (fv_set_max_lag)."""
    _fields_ = [("max_lag", ctypes.c_longlong), ("forced_commits", ctypes.c_longlong), ("pruned_states", ctypes.c_longlong),
                ("first_forced_time", ctypes.c_longlong), ("last_forced_time", ctypes.c_longlong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SumprodStats(ctypes.Structure):
    """fv_sumprod_stats: the last loglik / loglik_batch / posteriors call."""
    _fields_ = [("call_ms", ctypes.c_double), ("gpu_ms", ctypes.c_double), ("step_launches", ctypes.c_longlong),
                ("task_steps", ctypes.c_longlong), ("table_bytes_per_step", ctypes.c_longlong), ("device_bytes", ctypes.c_longlong),
                ("refine_columns", ctypes.c_longlong), ("refine_finite", ctypes.c_longlong), ("passes", ctypes.c_int),
                ("batch_cap", ctypes.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CountsStats(ctypes.Structure):
    """fv_counts_stats: the last expected_counts call."""
    _fields_ = [("call_ms", ctypes.c_double), ("gpu_ms", ctypes.c_double), ("sequences", ctypes.c_longlong),
                ("dead_sequences", ctypes.c_longlong), ("times", ctypes.c_longlong), ("step_launches", ctypes.c_longlong),
                ("task_steps", ctypes.c_longlong), ("xi_launches", ctypes.c_longlong), ("wide_times", ctypes.c_longlong),
                ("device_bytes", ctypes.c_longlong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FlatInfo(ctypes.Structure):
    """fv_flat_info: one right-hand pass of the flat schedule."""
    _fields_ = [("L", ctypes.c_int), ("R", ctypes.c_int), ("generation", ctypes.c_int), ("batch", ctypes.c_int),
                ("stream", ctypes.c_int), ("chain", ctypes.c_int), ("arg_row", ctypes.c_longlong)]


class PassInfo(ctypes.Structure):
    _fields_ = [("L", ctypes.c_int), ("R", ctypes.c_int), ("generation", ctypes.c_int), ("owner", ctypes.c_int)]


EXPORTS = ["fv_create", "fv_destroy", "fv_set_model", "fv_set_option", "fv_decode_full", "fv_decode_beam",
           "fv_decode_vanilla", "fv_decode_checkpoint", "fv_checkpoint_memory_bytes",
           "fv_last_stats", "fv_strerror", "fv_last_error_detail", "fv_reference_memory_bytes",
           "fv_comm_unique_id", "fv_comm_init", "fv_plan_passes", "fv_merge_paths", "fv_set_partition",
           "fv_create_multi", "fv_device_count", "fv_decode_full_batch", "fv_plan_passes_batch", "fv_decode_beam_batch",
           "fv_set_model_sparse", "fv_set_emissions", "fv_clear_emissions", "fv_plan_flat", "fv_set_emission_map",
           "fv_stream_open", "fv_stream_push", "fv_stream_push_emissions", "fv_stream_pending", "fv_stream_close",
           "fv_stream_abort", "fv_stream_last_stats",
           "fv_streams_open", "fv_streams_push", "fv_streams_push_emissions", "fv_streams_pending", "fv_streams_close",
           "fv_streams_abort", "fv_streams_end", "fv_streams_slot_stats", "fv_streams_last_stats",
           "fv_set_max_lag", "fv_last_lag_stats",
           "fv_loglik", "fv_loglik_batch", "fv_posteriors", "fv_last_sumprod_stats", "fv_set_sparse_sumprod",
           "fv_expected_counts", "fv_last_counts_stats"]
# include/flashvit_testing.h: hooks for the test suite, not part of the drop-in ABI above
TEST_EXPORTS = ["fv_test_forward", "fv_test_beam_step", "fv_test_beam_select", "fv_test_device_alloc", "fv_test_device_free",
                "fv_test_stage_emissions_ms", "fv_test_flat_poison", "fv_test_beam_forward", "fv_test_model_digest",
                "fv_test_sumprod_rows", "fv_test_sumprod_forms"]
# FV_SPF_* of include/flashvit_testing.h (test_sumprod_forms): three bits per family of sum-product step kernels, for NB = 1, 2, 4
# tasks at shift + 0, + 1, + 2
SPF_DENSE_SHIFT, SPF_CSR_FWD_LDS_SHIFT, SPF_CSR_FWD_MEM_SHIFT, SPF_CSR_BACK_LDS_SHIFT, SPF_CSR_BACK_MEM_SHIFT = 0, 3, 6, 9, 12


def spf_family(shift):
    """FV_SPF_FAMILY: the three bits of one family"""
    return 7 << shift


TIE_TAG = 1 << 30
# FV_TS_*: select-kernel instantiations reported by test_beam_select
TS_BITS = {"topb_select<4,listed>": 1 << 0, "topb_select<4,derived>": 1 << 1, "topb_select<16,listed>": 1 << 2,
           "topb_select<16,derived>": 1 << 3, "topb_select<64,listed>": 1 << 4, "topb_select<64,derived>": 1 << 5,
           "topb_select_cand<8,listed>": 1 << 6, "topb_select_cand<8,derived>": 1 << 7, "topb_select_cand<16,listed>": 1 << 8,
           "topb_select_cand<16,derived>": 1 << 9, "heap_build_all": 1 << 10}
TS_ALL = (1 << 11) - 1
CUT_THETA, CUT_STATE, CUT_NEXT, CUT_LIST, CUT_N, CUT_MARGIN, CUT_W = 0, 1, 2, 3, 4, 5, 8
BEAM_EXTRA = 32                        # entries beyond B a speculative member list can hold
SELECT_COUNTERS = (2, 5, 7, 9, 10, 11, 12, 13)


class ForwardPass(ctypes.Structure):
    """fv_test_pass: steps L+1 .. R from Pi (init_state < 0, L = 0) or from state init_state at time L - 1."""
    _fields_ = [("L", ctypes.c_int), ("R", ctypes.c_int), ("init_state", ctypes.c_int)]


class BeamPass(ctypes.Structure):
    """fv_test_beam_pass: one FLASH-BS pass [L, R] from init_state (< 0: Pi) to the fixed end state end_state."""
    _fields_ = [("L", ctypes.c_int), ("R", ctypes.c_int), ("init_state", ctypes.c_int), ("end_state", ctypes.c_int)]


class BeamTables(ctypes.Structure):
    """fv_test_beam_tables: where fv_test_beam_forward copies the per-step buffers (NULL: not wanted)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("scores", "bp", "cut", "member_val", "member_state", "doubt", "doubt_count",
                                               "slot_val", "slot_state", "path", "score", "gate", "variants", "selects")]


DOUBT_CAP = 1024                       # doubtful columns a step lists


class SelectSet(ctypes.Structure):
    """fv_test_select_set: one score row and, optionally, its candidate list."""
    _fields_ = [("scores", ctypes.c_void_p), ("cand", ctypes.c_void_p), ("cand_count", ctypes.c_int)]


class BeamSet(ctypes.Structure):
    """fv_test_beam_set: n entries (value, state) of one beam step's slot set."""
    _fields_ = [("val", ctypes.c_void_p), ("state", ctypes.c_void_p), ("n", ctypes.c_int)]

_lib = None


def load_library():
    """dlopen libflashvit.so (no GPU needed for that) and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    # FLASHVIT_TIMING_BUILD=1 (tools/ only): the build that keeps the result-changing timing switches of FV_OPT_DEBUG
    path = _build.HIP_TIMING_LIB if os.environ.get("FLASHVIT_TIMING_BUILD") == "1" else _build.HIP_LIB
    if not os.path.isfile(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(path)
    vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.fv_create.argtypes = [ctypes.POINTER(vp), ci]
    L.fv_create_multi.argtypes = [ctypes.POINTER(vp), vp, ci]
    L.fv_device_count.argtypes = []
    L.fv_destroy.argtypes = [vp]
    L.fv_destroy.restype = None
    L.fv_set_model.argtypes = [vp, vp, vp, vp, ci, ci]
    L.fv_set_model_sparse.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci]
    L.fv_set_option.argtypes = [vp, ci, cll]
    L.fv_set_emissions.argtypes = [vp, vp, ci, ci, cll]
    L.fv_clear_emissions.argtypes = [vp]
    L.fv_set_emission_map.argtypes = [vp, vp, ci]
    L.fv_stream_open.argtypes = [vp, cll, ci]
    L.fv_stream_push.argtypes = [vp, vp, ci, vp, ctypes.POINTER(cll)]
    L.fv_stream_push_emissions.argtypes = [vp, vp, ci, ci, cll, vp, ctypes.POINTER(cll)]
    L.fv_stream_pending.argtypes = [vp]
    L.fv_stream_pending.restype = cll
    L.fv_stream_close.argtypes = [vp, vp, ctypes.POINTER(cll), ctypes.POINTER(ctypes.c_float)]
    L.fv_stream_abort.argtypes = [vp]
    L.fv_stream_last_stats.argtypes = [vp, ctypes.POINTER(StreamStats)]
    L.fv_streams_open.argtypes = [vp, ci, cll, ci]
    L.fv_streams_push.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.fv_streams_push_emissions.argtypes = [vp, vp, ci, vp, ci, vp, cll, vp, vp, vp, vp]
    L.fv_streams_pending.argtypes = [vp, ci]
    L.fv_streams_pending.restype = cll
    L.fv_streams_close.argtypes = [vp, ci, vp, ctypes.POINTER(cll), ctypes.POINTER(ctypes.c_float)]
    L.fv_streams_abort.argtypes = [vp, ci]
    L.fv_streams_end.argtypes = [vp]
    L.fv_streams_slot_stats.argtypes = [vp, ci, ctypes.POINTER(StreamStats)]
    L.fv_streams_last_stats.argtypes = [vp, ctypes.POINTER(StreamsStats)]
    L.fv_set_max_lag.argtypes = [vp, cll]
    L.fv_last_lag_stats.argtypes = [vp, ci, ctypes.POINTER(LagStats)]
    L.fv_loglik.argtypes = [vp, vp, ci, ctypes.POINTER(ctypes.c_double)]
    L.fv_loglik_batch.argtypes = [vp, vp, vp, ci, vp, vp]
    L.fv_posteriors.argtypes = [vp, vp, ci, vp, cll, vp, ctypes.POINTER(ctypes.c_double)]
    L.fv_last_sumprod_stats.argtypes = [vp, ctypes.POINTER(SumprodStats)]
    L.fv_test_sumprod_rows.argtypes = [vp, vp, ci, vp, vp]
    L.fv_set_sparse_sumprod.argtypes = [vp, ci]
    L.fv_expected_counts.argtypes = [vp, vp, vp, ci, vp, cll, vp, vp, vp, vp, vp]
    L.fv_last_counts_stats.argtypes = [vp, ctypes.POINTER(CountsStats)]
    L.fv_test_sumprod_forms.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong)]
    L.fv_test_device_alloc.argtypes = [vp, ctypes.c_size_t, vp, ctypes.POINTER(vp)]
    L.fv_test_device_free.argtypes = [vp, vp]
    L.fv_test_stage_emissions_ms.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    L.fv_decode_full.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    L.fv_decode_beam.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
    L.fv_decode_full_batch.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp]
    L.fv_decode_beam_batch.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]
    L.fv_plan_passes_batch.argtypes = [vp, ci, ci, ci, ctypes.POINTER(PassInfo), ci]
    L.fv_decode_vanilla.argtypes = [vp, vp, ci, vp, vp]
    L.fv_decode_checkpoint.argtypes = [vp, vp, ci, ci, vp, vp]
    L.fv_checkpoint_memory_bytes.argtypes = [ci, ci, ci]
    L.fv_checkpoint_memory_bytes.restype = ctypes.c_longlong
    L.fv_last_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    L.fv_strerror.argtypes = [ci]
    L.fv_strerror.restype = ctypes.c_char_p
    L.fv_last_error_detail.argtypes = [vp]
    L.fv_last_error_detail.restype = ctypes.c_char_p
    L.fv_reference_memory_bytes.argtypes = [ci, ci, ci, ci]
    L.fv_reference_memory_bytes.restype = cll
    L.fv_comm_unique_id.argtypes = [vp]
    L.fv_comm_init.argtypes = [vp, ci, ci, vp]
    L.fv_set_partition.argtypes = [vp, ci, ci]
    L.fv_plan_passes.argtypes = [ci, ci, ci, ci, ctypes.POINTER(PassInfo), ci]
    L.fv_merge_paths.argtypes = [ci, ci, ci, vp, vp]
    L.fv_plan_flat.argtypes = [ci, ci, ci, ci, ctypes.POINTER(FlatInfo), ci]
    L.fv_test_flat_poison.argtypes = [vp, ci]
    L.fv_test_model_digest.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, ctypes.c_char_p, ci]
    L.fv_test_forward.argtypes = [vp, vp, ci, ctypes.POINTER(ForwardPass), ci, vp, vp, ctypes.POINTER(ctypes.c_ulonglong)]
    cf = ctypes.c_float
    L.fv_test_beam_step.argtypes = [vp, ci, ctypes.POINTER(BeamSet), ci, vp, ci, cf, cf, ci, vp, vp, vp, ctypes.POINTER(ci),
                                    vp, vp, vp, vp, ctypes.POINTER(ctypes.c_ulonglong)]
    L.fv_test_beam_select.argtypes = [vp, ci, ci, ci, ctypes.POINTER(SelectSet), ci, cf, cf, vp, ci, ctypes.POINTER(ci), vp,
                                      vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_ulonglong)]
    L.fv_test_beam_forward.argtypes = [vp, vp, ci, ci, ctypes.POINTER(BeamPass), ci, ctypes.POINTER(BeamTables)]
    _lib = L
    return L


class FlashVitError(RuntimeError):
    def __init__(self, rc, detail=""):
        msg = load_library().fv_strerror(rc).decode()
        super().__init__(f"flashvit: {msg} ({rc})" + (f": {detail}" if detail else ""))
        self.rc = rc


def plan_passes(T, n_split, mode=MODE_REFERENCE, nranks=1):
    """Host-side schedule (no GPU): list of (L, R, generation, owner)."""
    L = load_library()
    n = L.fv_plan_passes(T, n_split, mode, nranks, None, 0)
    if n < 0:
        raise FlashVitError(n)
    buf = (PassInfo * n)()
    L.fv_plan_passes(T, n_split, mode, nranks, buf, n)
    return [(p.L, p.R, p.generation, p.owner) for p in buf]


def plan_flat(T, n_split, batch_cap=4, nstreams=3):
    """Flat schedule of OPT_FLAT_GENERATIONS (no GPU): list of dicts L, R, generation, batch, stream, chain, arg_row."""
    L = load_library()
    n = L.fv_plan_flat(T, n_split, batch_cap, nstreams, None, 0)
    if n < 0:
        raise FlashVitError(n)
    buf = (FlatInfo * max(n, 1))()
    L.fv_plan_flat(T, n_split, batch_cap, nstreams, buf, n)
    return [{k: getattr(buf[i], k) for k, _ in FlatInfo._fields_} for i in range(n)]


def plan_passes_batch(lengths, n_split, mode=MODE_REFERENCE):
    """Host-side schedule of decode_full_batch (no GPU): list of (L, R, generation, sequence index), L and R on the
    concatenated time axis (sequence s starts at sum(lengths[:s]))."""
    L = load_library()
    lens = np.ascontiguousarray(lengths, dtype=np.int32)
    n = L.fv_plan_passes_batch(_p(lens), lens.size, n_split, mode, None, 0)
    if n < 0:
        raise FlashVitError(n)
    buf = (PassInfo * n)()
    L.fv_plan_passes_batch(_p(lens), lens.size, n_split, mode, buf, n)
    return [(p.L, p.R, p.generation, p.owner) for p in buf]


def merge_paths(T, n_split, nranks, gathered):
    """The product's post-all-gather merge (host C++), callable without a GPU."""
    g = np.ascontiguousarray(gathered, dtype=np.int32).reshape(nranks * T)
    out = np.empty(T, dtype=np.int32)
    rc = load_library().fv_merge_paths(T, n_split, nranks, _p(g), _p(out))
    if rc < 0:
        raise FlashVitError(rc)
    return out


def reference_memory_bytes(K, T, n_split, beam=0):
    return int(load_library().fv_reference_memory_bytes(K, T, n_split, beam))


def checkpoint_memory_bytes(K, T, step=0):
    return int(load_library().fv_checkpoint_memory_bytes(K, T, step))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _is_torch_tensor(x):
    """whether x is a torch.Tensor, without importing torch for anything that is not one"""
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _ob_arg(ob, T):
    """(keep-alive array, pointer, length) of a decode's observations: an int sequence, or None with T = the number of staged emission
    rows to decode (fv_set_emissions)."""
    if ob is None:
        if T is None:
            raise ValueError("ob=None decodes the staged emission scores: give T, the number of times")
        return None, None, int(T)
    ob = np.ascontiguousarray(ob, dtype=np.int32)
    if T is not None and int(T) != ob.size:
        raise ValueError("T differs from the length of ob")
    return ob, _p(ob), ob.size


def _batch_arg(obs, lengths):
    """(keep-alive array, pointer, offsets) of a batch decode's observations: a list of int sequences, or None with
    lengths = the number of staged emission rows of every sequence (laid end to end in the staged block)."""
    if obs is None:
        if lengths is None:
            raise ValueError("obs=None decodes the staged emission scores: give lengths")
        sizes, ob, ptr = [int(n) for n in lengths], None, None
    else:
        if lengths is not None:
            raise ValueError("lengths goes with obs=None")
        seqs = [np.ascontiguousarray(o, dtype=np.int32).reshape(-1) for o in obs]
        sizes = [o.size for o in seqs]
        ob = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.int32)
        ptr = _p(ob)
    offsets = np.zeros(len(sizes) + 1, dtype=np.int64)
    if sizes:
        offsets[1:] = np.cumsum(sizes)
    return ob, ptr, offsets


def _emission_arg(scores, ld, who):
    """(keep-alive object, pointer, EMIS_LOG_* code, rows, pitch) of a block of emission scores in the three forms
    set_emissions and stream_push document: a numpy array, a torch tensor, (device_pointer, dtype, T, ld)."""
    if isinstance(scores, tuple):
        ptr, dtype, T, pitch = scores
        if ld is not None:
            pitch = ld
        if isinstance(dtype, (type, np.dtype, str)):
            dtype = _EMIS_OF_NUMPY.get(np.dtype(dtype), -1)
        return None, ctypes.c_void_p(int(ptr)), int(dtype), int(T), int(pitch)
    if _is_torch_tensor(scores):
        import torch
        codes = {torch.float16: EMIS_LOG_F16, torch.bfloat16: EMIS_LOG_BF16, torch.float32: EMIS_LOG_F32, torch.float64: EMIS_LOG_F64}
        if scores.dim() != 2 or scores.dtype not in codes or scores.stride(1) != 1 or scores.shape[0] < 1 or scores.shape[1] < 1:
            raise TypeError(who + ": a torch tensor must be 2-D, float16 / bfloat16 / float32 / float64, with stride(1) == 1")
        pitch = scores.stride(0) if ld is None else int(ld)
        if scores.shape[0] == 1:
            pitch = max(pitch, scores.shape[1])         # (one row: its stride is arbitrary and never used)
        if scores.is_cuda:
            torch.cuda.current_stream(scores.device).synchronize()      # the C contract: the producer has finished
        return scores, ctypes.c_void_p(scores.data_ptr()), codes[scores.dtype], scores.shape[0], pitch
    a = np.asarray(scores)
    if a.ndim != 2 or a.dtype not in _EMIS_OF_NUMPY:
        raise TypeError(who + ": a 2-D float16, float32 or float64 array, a torch tensor, or (device_pointer, dtype, T, ld)")
    a = np.ascontiguousarray(a)
    pitch = a.shape[1] if ld is None else int(ld)
    if pitch > a.shape[1] and a.shape[0] > 1:
        raise ValueError(who + ": ld exceeds the row length of the array")
    return a, _p(a), _EMIS_OF_NUMPY[a.dtype], a.shape[0], pitch


def dense_to_csr(A):
    """(indptr int64[K + 1], indices int32[nnz], data float32[nnz]) of a dense K x K matrix, by row with ascending
    columns: what set_model_sparse takes.  Entries equal to 0 are left out (NaN is kept, so that the library sees it)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    assert A.ndim == 2 and A.shape[0] == A.shape[1]
    rows, cols = np.nonzero(A != 0)              # row-major order: ascending columns inside a row
    indptr = np.zeros(A.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=A.shape[0]), out=indptr[1:])
    return indptr, cols.astype(np.int32), A[rows, cols]


MODEL_DIGESTS_DENSE = ("h64", "h32", "h16", "hq", "sp", "sp_off", "sp_nwb", "b64", "b32", "pi64")
MODEL_DIGESTS_CSR = ("ck", "cq", "c64", "off", "nwb", "rlog", "b64", "b32", "pi64")
MODEL_PARAMS = ("window16", "windowq", "qscale", "density", "any_big")


def test_model_digest(A, B, Pi):
    """fv_test_model_digest (no GPU): the host builder of set_model (A: a dense K x K matrix) or of set_model_sparse (A: the
    tuple (indptr, indices, data)) alone.  Returns (rc, detail, digests, params): the builder's return code and refusal
    sentence, the FNV-1a digest of every host table by the names of MODEL_DIGESTS_DENSE / _CSR, and MODEL_PARAMS as floats."""
    B = np.ascontiguousarray(B, dtype=np.float32)
    Pi = np.ascontiguousarray(Pi, dtype=np.float32)
    K, M = B.shape
    if isinstance(A, tuple):
        indptr, indices, data = (np.ascontiguousarray(a, dtype=t) for a, t in zip(A, (np.int64, np.int32, np.float32)))
        args, names = (None, _p(indptr), _p(indices), _p(data)), MODEL_DIGESTS_CSR
    else:
        A = np.ascontiguousarray(A, dtype=np.float32)
        assert A.shape == (K, K)
        args, names = (_p(A), None, None, None), MODEL_DIGESTS_DENSE
    digests = np.zeros(len(names), dtype=np.uint64)
    params = np.zeros(len(MODEL_PARAMS), dtype=np.float64)
    detail = ctypes.create_string_buffer(512)
    rc = load_library().fv_test_model_digest(*args, _p(B), _p(Pi), K, M, _p(digests), _p(params), detail, len(detail))
    return rc, detail.value.decode(), dict(zip(names, (int(d) for d in digests))), dict(zip(MODEL_PARAMS, params.tolist()))


class FlashViterbi:
    """One decoder context on one GPU.  Mirrors the reference program's life cycle:
    create_vit() -> calc() -> printAns() becomes set_model() -> decode_*() -> returned path."""

    def __init__(self, device=0):
        """device: one device id, or a list of ids for a single-process multi-device context (fv_create_multi;
        an id may repeat: the members then share that GPU and gather by device-to-device copies)."""
        self._L = load_library()
        h = ctypes.c_void_p()
        if isinstance(device, (list, tuple)):
            devs = np.ascontiguousarray(device, dtype=np.int32)
            rc = self._L.fv_create_multi(ctypes.byref(h), _p(devs), devs.size)
        else:
            rc = self._L.fv_create(ctypes.byref(h), device)
        if rc != 0:
            raise FlashVitError(rc, "fv_create (is a GPU visible? there is no CPU fallback)")
        self._h = h
        self.K = self.M = 0
        self.P = 0                          # classes of the emission map in force (set_emission_map); 0: none

    def close(self):
        if getattr(self, "_h", None):
            self._L.fv_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc < 0:
            raise FlashVitError(rc, self._L.fv_last_error_detail(self._h).decode())
        return rc

    def set_option(self, key, value):
        self._check(self._L.fv_set_option(self._h, key, int(value)))

    def set_model(self, A, B, Pi):
        A = np.ascontiguousarray(A, dtype=np.float32)
        B = np.ascontiguousarray(B, dtype=np.float32)
        Pi = np.ascontiguousarray(Pi, dtype=np.float32)
        K, M = B.shape
        assert A.shape == (K, K) and Pi.shape == (K,)
        self._check(self._L.fv_set_model(self._h, _p(A), _p(B), _p(Pi), K, M))
        self.K, self.M, self.P = K, M, 0

    def set_model_sparse(self, indptr, indices, data, B, Pi):
        """fv_set_model_sparse: the transition matrix in CSR form by source state (indptr[K + 1], ascending column
        indices per row, values; dense_to_csr makes them from a dense matrix).  No K x K array exists on this path."""
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float32)
        B = np.ascontiguousarray(B, dtype=np.float32)
        Pi = np.ascontiguousarray(Pi, dtype=np.float32)
        K, M = B.shape
        assert indptr.shape == (K + 1,) and Pi.shape == (K,) and indices.shape == data.shape and indices.ndim == 1
        # (the array lengths are the wrapper's to check: the library reads row_ptr[K] entries of both)
        assert indptr[-1] <= indices.size, "indptr[K] exceeds the number of stored entries"
        self._check(self._L.fv_set_model_sparse(self._h, _p(indptr), _p(indices), _p(data), _p(B), _p(Pi), K, M))
        self.K, self.M, self.P = K, M, 0

    def set_emission_map(self, pdf_of_state, P=None):
        """fv_set_emission_map: the K states share P score classes, state i scoring as class pdf_of_state[i]; set_emissions
        then takes rows of P scores.  P defaults to max(pdf_of_state) + 1.  None clears the map.  Either way the staged
        rows are dropped.  self.P is the class count in force (0: no map)."""
        if pdf_of_state is None:
            self._check(self._L.fv_set_emission_map(self._h, None, 0))
            self.P = 0
            return
        m = np.ascontiguousarray(pdf_of_state, dtype=np.int32)
        if m.shape != (self.K,):
            raise ValueError("set_emission_map: one entry per state of the model")
        P = int(m.max()) + 1 if P is None else int(P)
        self._check(self._L.fv_set_emission_map(self._h, _p(m), P))
        self.P = P

    def set_emissions(self, scores, ld=None):
        """fv_set_emissions: per-time log emission scores, row t = the K scores of time t (the P class scores while an
        emission map is set).  `scores` is a 2-D float16, float32 or float64 numpy array [T, >= K] (ld: its row pitch in
        elements, default its width; columns beyond K are not interpreted); a 2-D torch tensor of dtype float16,
        bfloat16, float32 or float64 with stride(1) == 1, on the CPU or on this context's GPU (ld = stride(0), so a
        column slice of a wider tensor is staged without a copy; the tensor's current stream is synchronised first); or
        a tuple (device_pointer:int, dtype, T, ld) for a block already on this context's GPU (dtype: np.float16 /
        np.float32 / np.float64 or an EMIS_LOG_* code; its producer must have finished).  Afterwards every decode_* and
        test_forward takes ob=None."""
        keep, ptr, code, T, pitch = _emission_arg(scores, ld, "set_emissions")
        self._check(self._L.fv_set_emissions(self._h, ptr, code, T, pitch))

    def clear_emissions(self):
        self._check(self._L.fv_clear_emissions(self._h))

    # ---- fv_stream_*: the online decode.  One stream per context; while it is open the other calls raise ERR_STATE.

    def stream_open(self, lag_rows_hint=0, check_every=0):
        """fv_stream_open: lag_rows_hint arg rows at first (0: a default), a check every check_every steps (1..64, 0: the default)."""
        self._check(self._L.fv_stream_open(self._h, int(lag_rows_hint), int(check_every)))

    def stream_push(self, ob=None, scores=None, ld=None):
        """fv_stream_push (ob: the symbols of the next times) or fv_stream_push_emissions (scores: their score rows, in
        the forms set_emissions takes — a numpy array, a torch tensor on the CPU or on this context's GPU, or
        (device_pointer, dtype, n, ld)).  Returns the piece of the path this push committed, int32, possibly empty.  A
        refused push raises FlashVitError and consumes nothing; ERR_NO_PRED means the stream is dead."""
        if (ob is None) == (scores is None):
            raise ValueError("stream_push: either ob or scores")
        done = ctypes.c_longlong(0)
        room = max(int(self._L.fv_stream_pending(self._h)), 0)
        if ob is not None:
            ob = np.ascontiguousarray(ob, dtype=np.int32).reshape(-1)
            piece = np.empty(room + max(ob.size, 1), dtype=np.int32)
            self._check(self._L.fv_stream_push(self._h, _p(ob), ob.size, _p(piece), ctypes.byref(done)))
        else:
            keep, ptr, code, n, pitch = _emission_arg(scores, ld, "stream_push")
            piece = np.empty(room + max(n, 1), dtype=np.int32)
            self._check(self._L.fv_stream_push_emissions(self._h, ptr, code, n, pitch, _p(piece), ctypes.byref(done)))
        return piece[:done.value].copy()

    def stream_pending(self):
        """fv_stream_pending: times consumed and not yet committed (< 0: no stream)."""
        return int(self._L.fv_stream_pending(self._h))

    def stream_close(self):
        """fv_stream_close: (the last piece, the score, rc).  ERR_NO_PRED is returned, not raised, as decode_full_batch
        reports it: the piece then holds what the library delivered (nothing for a dead stream)."""
        piece = np.empty(max(int(self._L.fv_stream_pending(self._h)), 1), dtype=np.int32)
        n = ctypes.c_longlong(0)
        score = ctypes.c_float(0)
        rc = self._L.fv_stream_close(self._h, _p(piece), ctypes.byref(n), ctypes.byref(score))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return piece[:n.value].copy(), np.float32(score.value), rc

    def stream_abort(self):
        self._check(self._L.fv_stream_abort(self._h))

    def stream_stats(self):
        s = StreamStats()
        self._check(self._L.fv_stream_last_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    # ---- fv_streams_*: a set of online streams ("slots") on one context, the slots of one push call stepped together.
    # A set and the single stream exclude each other.

    def streams_open(self, nslots, lag_rows_hint=0, check_every=0):
        """fv_streams_open: nslots slots (1..64), lag_rows_hint and check_every as stream_open, for every slot."""
        self._check(self._L.fv_streams_open(self._h, int(nslots), int(lag_rows_hint), int(check_every)))

    def streams_push(self, ids, obs=None, scores=None, ld=None):
        """fv_streams_push (obs: one int sequence per named slot) or fv_streams_push_emissions (scores: one 2-D array of
        score rows per named slot, packed into one block; or (block, lengths), block in the forms set_emissions takes with
        slot ids[q]'s rows laid end to end in it).  Returns (pieces, statuses): per named slot the piece of the path this
        call committed (int32, possibly empty) and FV_OK or ERR_NO_PRED — a dead slot is reported, not raised, as
        decode_full_batch reports it.  A refused call raises FlashVitError and consumes nothing in any slot."""
        if (obs is None) == (scores is None):
            raise ValueError("streams_push: either obs or scores")
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if obs is not None:
            ob, ptr, offsets = _batch_arg(obs, None)
        elif isinstance(scores, tuple) and len(scores) == 2:
            block, lengths = scores
            _, _, offsets = _batch_arg(None, lengths)
            keep, ptr, code, n, pitch = _emission_arg(block, ld, "streams_push")
        else:
            blocks = [np.asarray(b) for b in scores]
            _, _, offsets = _batch_arg(None, [b.shape[0] for b in blocks])
            keep, ptr, code, n, pitch = _emission_arg(np.concatenate(blocks) if blocks else np.zeros((0, 0), np.float32), ld, "streams_push")
        if offsets.size != ids.size + 1:
            raise ValueError("streams_push: one sequence per named slot")
        sizes, pending, room = offsets.tolist(), self._L.fv_streams_pending, [0]
        for q, i in enumerate(ids.tolist()):
            room.append(room[-1] + max(pending(self._h, i), 0) + max(sizes[q + 1] - sizes[q], 1))
        room = np.array(room, dtype=np.int64)
        path = np.empty(max(int(room[-1]), 1), dtype=np.int32)
        done = np.zeros(max(ids.size, 1), dtype=np.int64)
        status = np.zeros(max(ids.size, 1), dtype=np.int32)
        if obs is not None:
            rc = self._L.fv_streams_push(self._h, _p(ids), ids.size, ptr, _p(offsets), _p(path), _p(room), _p(done), _p(status))
        else:
            rc = self._L.fv_streams_push_emissions(self._h, _p(ids), ids.size, ptr, code, _p(offsets), pitch, _p(path), _p(room),
                                                   _p(done), _p(status))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return ([path[room[q]:room[q] + done[q]].copy() for q in range(ids.size)], [int(x) for x in status[:ids.size]])

    def streams_pending(self, id):
        """fv_streams_pending: times slot id consumed and has not yet committed (< 0: no set, or no such slot)."""
        return int(self._L.fv_streams_pending(self._h, int(id)))

    def streams_close(self, id):
        """fv_streams_close: (the last piece, the score, rc) of slot id's sequence, as stream_close; the slot is empty again."""
        piece = np.empty(max(int(self._L.fv_streams_pending(self._h, int(id))), 1), dtype=np.int32)
        n = ctypes.c_longlong(0)
        score = ctypes.c_float(0)
        rc = self._L.fv_streams_close(self._h, int(id), _p(piece), ctypes.byref(n), ctypes.byref(score))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return piece[:n.value].copy(), np.float32(score.value), rc

    def streams_abort(self, id):
        self._check(self._L.fv_streams_abort(self._h, int(id)))

    def streams_end(self):
        self._check(self._L.fv_streams_end(self._h))

    def streams_slot_stats(self, id):
        s = StreamStats()
        self._check(self._L.fv_streams_slot_stats(self._h, int(id), ctypes.byref(s)))
        return s.as_dict()

    def streams_stats(self):
        s = StreamsStats()
        self._check(self._L.fv_streams_last_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    # ---- fv_set_max_lag: streams and sets opened afterwards commit at the latest max_lag steps behind a check (inexact)

    def set_max_lag(self, max_lag):
        """fv_set_max_lag: 0 unbounded (the default); >= 1: a check that finds more than one ancestor max_lag or more steps
        past the anchor forces the commit of the best state's ancestor and prunes the other states."""
        self._check(self._L.fv_set_max_lag(self._h, int(max_lag)))

    def lag_stats(self, slot=None):
        """fv_last_lag_stats of the single stream (slot=None) or of a slot of the set: a dict of LagStats' members."""
        s = LagStats()
        self._check(self._L.fv_last_lag_stats(self._h, -1 if slot is None else int(slot), ctypes.byref(s)))
        return s.as_dict()

    # ---- fv_loglik / fv_posteriors: forward-backward in float64

    def loglik(self, ob=None, T=None):
        """fv_loglik: log P(ob | model) as a float; -inf (no exception) when the model gives the sequence probability 0.
        ob=None with T=...: on the first T rows staged by set_emissions."""
        ob, ptr, T = _ob_arg(ob, T)
        out = ctypes.c_double(0)
        rc = self._L.fv_loglik(self._h, ptr, T, ctypes.byref(out))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return float(out.value)

    def loglik_batch(self, obs, lengths=None):
        """fv_loglik_batch: obs is a list of int sequences (lengths >= 1, may differ).  Returns (logliks: float64 array,
        statuses: int32 array), per sequence what loglik gives for it alone (the same bits); a sequence of probability 0
        reports -inf and ERR_NO_PRED and does not raise.  obs=None with lengths=[...]: as decode_full_batch."""
        ob, ptr, offsets = _batch_arg(obs, lengths)
        nseq = offsets.size - 1
        ll = np.zeros(max(nseq, 1), dtype=np.float64)
        statuses = np.zeros(max(nseq, 1), dtype=np.int32)
        rc = self._L.fv_loglik_batch(self._h, ptr, _p(offsets), nseq, _p(ll), _p(statuses))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return ll[:nseq], statuses[:nseq]

    def posteriors(self, ob=None, T=None, want_gamma=True, out=None):
        """fv_posteriors: returns (gamma, path, loglik).  gamma is a float32 array [T, K] of state posteriors (None with
        want_gamma=False, or with out=...), path the int32 posterior decoding, loglik a float.  out: a device pointer
        (from test_device_alloc or a torch tensor's data_ptr()) or (pointer, ld) that receives gamma on the device, row
        pitch ld (default K) in elements.  A sequence of probability 0 gives (None, a path of -1, -inf) and does not raise."""
        ob, ptr, T = _ob_arg(ob, T)
        path = np.empty(T, dtype=np.int32)
        ll = ctypes.c_double(0)
        gamma, gptr, ld = None, None, self.K
        if out is not None:
            gptr, ld = out if isinstance(out, tuple) else (out, self.K)
            gptr = ctypes.c_void_p(int(gptr))
        elif want_gamma:
            gamma = np.empty((T, self.K), dtype=np.float32)
            gptr = _p(gamma)
        rc = self._L.fv_posteriors(self._h, ptr, T, gptr, int(ld), _p(path), ctypes.byref(ll))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return (None if rc == ERR_NO_PRED else gamma), path, float(ll.value)

    def sumprod_stats(self):
        """fv_last_sumprod_stats: a dict of SumprodStats' members for the last loglik / loglik_batch / posteriors."""
        s = SumprodStats()
        self._check(self._L.fv_last_sumprod_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def test_sumprod_rows(self, ob=None, T=None):
        """fv_test_sumprod_rows: (alpha[T, K], beta[T, K], rc) of fv_posteriors' two passes, float64."""
        ob, ptr, T = _ob_arg(ob, T)
        alpha = np.empty((T, self.K), dtype=np.float64)
        beta = np.empty((T, self.K), dtype=np.float64)
        rc = self._L.fv_test_sumprod_rows(self._h, ptr, T, _p(alpha), _p(beta))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return alpha, beta, rc

    def set_sparse_sumprod(self, on):
        """fv_set_sparse_sumprod: 0 (the default) / 1: loglik, loglik_batch and posteriors run on a model set by
        set_model_sparse (refused under 0); kept across set_model / set_model_sparse, no effect on a model set by set_model."""
        self._check(self._L.fv_set_sparse_sumprod(self._h, int(on)))

    def test_sumprod_forms(self):
        """fv_test_sumprod_forms: the SPF_* bits of the step kernels the last loglik / loglik_batch / posteriors /
        test_sumprod_rows launched."""
        mask = ctypes.c_ulonglong(0)
        self._check(self._L.fv_test_sumprod_forms(self._h, ctypes.byref(mask)))
        return int(mask.value)

    # ---- fv_expected_counts: the Baum-Welch E-step in float64

    def expected_counts(self, obs=None, lengths=None, want_trans=True, trans_out=None):
        """fv_expected_counts: obs is a list of int sequences (lengths >= 1, may differ); obs=None with lengths=[...]: on
        the staged emission rows, as loglik_batch.  Returns a dict of float64 arrays: trans [K, K] (None with
        want_trans=False or with trans_out=...), emit [K, M] (None with obs=None), init [K], occ [K], loglik [nseq], and
        status (int32 [nseq]).  trans_out: a device pointer or (pointer, ld) that receives trans on the device, row pitch
        ld (default K) in elements.  A sequence of probability 0 reports -inf and ERR_NO_PRED, contributes nothing and
        does not raise."""
        ob, ptr, offsets = _batch_arg(obs, lengths)
        nseq = offsets.size - 1
        K = self.K
        trans, tptr, ld = None, None, K
        if trans_out is not None:
            tptr, ld = trans_out if isinstance(trans_out, tuple) else (trans_out, K)
            tptr = ctypes.c_void_p(int(tptr))
        elif want_trans:
            trans = np.empty((K, K), dtype=np.float64)
            tptr = _p(trans)
        emit = None if ob is None else np.empty((K, self.M), dtype=np.float64)
        init, occ = np.empty(K, dtype=np.float64), np.empty(K, dtype=np.float64)
        ll = np.zeros(max(nseq, 1), dtype=np.float64)
        statuses = np.zeros(max(nseq, 1), dtype=np.int32)
        rc = self._L.fv_expected_counts(self._h, ptr, _p(offsets), nseq, tptr, int(ld), None if emit is None else _p(emit),
                                        _p(init), _p(occ), _p(ll), _p(statuses))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return dict(trans=trans, emit=emit, init=init, occ=occ, loglik=ll[:nseq], status=statuses[:nseq])

    def counts_stats(self):
        """fv_last_counts_stats: a dict of CountsStats' members for the last expected_counts."""
        s = CountsStats()
        self._check(self._L.fv_last_counts_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def decode_full(self, ob, n_split=1, mode=MODE_REFERENCE, T=None):
        """ob=None with T=...: decode the first T rows staged by set_emissions (so for every decode_* below)."""
        ob, ptr, T = _ob_arg(ob, T)
        path = np.empty(T, dtype=np.int32)
        score = ctypes.c_float(0)
        rc = self._check(self._L.fv_decode_full(self._h, ptr, T, n_split, mode, _p(path), ctypes.byref(score)))
        return path, np.float32(score.value), rc

    def decode_full_batch(self, obs, n_split=1, mode=MODE_REFERENCE, lengths=None):
        """fv_decode_full_batch: obs is a list of int sequences (lengths may differ) for the model of this context.
        Returns (paths: list of int32 arrays, scores: float32 array, statuses: int32 array), per sequence what
        decode_full returns for it alone.  A sequence whose path has an entry without a finite predecessor reports
        ERR_NO_PRED in `statuses` (its path holds the -1 entries) and does not raise: the other sequences' results
        stand.  Every other negative return raises FlashVitError.  obs=None with lengths=[...]: sequence s is the next
        lengths[s] rows of the block staged by set_emissions."""
        ob, ptr, offsets = _batch_arg(obs, lengths)
        nseq = offsets.size - 1
        path = np.empty(max(int(offsets[-1]), 1), dtype=np.int32)
        scores = np.zeros(nseq, dtype=np.float32)
        statuses = np.zeros(nseq, dtype=np.int32)
        rc = self._L.fv_decode_full_batch(self._h, ptr, _p(offsets), nseq, n_split, mode, _p(path), _p(scores), _p(statuses))
        if rc != ERR_NO_PRED:
            self._check(rc)
        return [path[offsets[s]:offsets[s + 1]].copy() for s in range(nseq)], scores, statuses

    def decode_beam(self, ob, n_split, beam, mode=MODE_REFERENCE, T=None):
        ob, ptr, T = _ob_arg(ob, T)
        path = np.empty(T, dtype=np.int32)
        score = ctypes.c_float(0)
        rc = self._check(self._L.fv_decode_beam(self._h, ptr, T, n_split, beam, mode, _p(path), ctypes.byref(score)))
        return path, np.float32(score.value), rc

    def decode_beam_batch(self, obs, n_split, beam, mode=MODE_REFERENCE, lengths=None):
        """fv_decode_beam_batch: obs is a list of int sequences (lengths may differ) for the model of this context.
        Returns (paths: list of int32 arrays, scores: float32 array, statuses: int32 array), per sequence what
        decode_beam returns for it alone: a sequence with a beam miss reports WARN_BEAM_MISS in `statuses` and its path
        holds the -1 entries.  Negative returns raise FlashVitError.  obs=None with lengths=[...]: as decode_full_batch."""
        ob, ptr, offsets = _batch_arg(obs, lengths)
        nseq = offsets.size - 1
        path = np.empty(max(int(offsets[-1]), 1), dtype=np.int32)
        scores = np.zeros(nseq, dtype=np.float32)
        statuses = np.zeros(nseq, dtype=np.int32)
        self._check(self._L.fv_decode_beam_batch(self._h, ptr, _p(offsets), nseq, n_split, beam, mode, _p(path),
                                                 _p(scores), _p(statuses)))
        return [path[offsets[s]:offsets[s + 1]].copy() for s in range(nseq)], scores, statuses

    def decode_vanilla(self, ob, T=None):
        ob, ptr, T = _ob_arg(ob, T)
        path = np.empty(T, dtype=np.int32)
        score = ctypes.c_float(0)
        rc = self._check(self._L.fv_decode_vanilla(self._h, ptr, T, _p(path), ctypes.byref(score)))
        return path, np.float32(score.value), rc

    def decode_checkpoint(self, ob, step=0, T=None):
        ob, ptr, T = _ob_arg(ob, T)
        path = np.empty(T, dtype=np.int32)
        score = ctypes.c_float(0)
        rc = self._check(self._L.fv_decode_checkpoint(self._h, ptr, T, step, _p(path), ctypes.byref(score)))
        return path, np.float32(score.value), rc

    def test_flat_poison(self, t):
        """fv_test_flat_poison: position t of the snapshot a flat decode speculates from holds a wrong state (t = -1 clears)."""
        self._check(self._L.fv_test_flat_poison(self._h, int(t)))

    def test_device_alloc(self, host_array):
        """fv_test_device_alloc: a device copy of a numpy array on this context's GPU; returns the pointer as an int
        (release it with test_device_free)."""
        a = np.ascontiguousarray(host_array)
        out = ctypes.c_void_p()
        self._check(self._L.fv_test_device_alloc(self._h, a.nbytes, _p(a), ctypes.byref(out)))
        return int(out.value)

    def test_device_free(self, ptr):
        self._check(self._L.fv_test_device_free(self._h, ctypes.c_void_p(int(ptr))))

    def test_stage_emissions_ms(self, ptr, dtype, T, ld, reps):
        """fv_test_stage_emissions_ms: mean milliseconds per launch of the staging kernel over the device block at ptr
        (device events around reps launches back to back); dtype as in set_emissions' tuple form.  While an emission
        map is set it is the tied form over a T x P block.  Nothing is staged afterwards."""
        ms = ctypes.c_float(0)
        code = dtype if isinstance(dtype, int) else _EMIS_OF_NUMPY.get(np.dtype(dtype), -1)
        self._check(self._L.fv_test_stage_emissions_ms(self._h, ctypes.c_void_p(int(ptr)), int(code), int(T), int(ld), int(reps), ctypes.byref(ms)))
        return float(ms.value)

    def test_forward(self, ob, passes, bp_fill=-2, T=None):
        """fv_test_forward: passes = [(L, R, init_state)], run as one generation of full-state passes.  Returns
        (rows[npasses, K] float32, bp[T, K] int32, variants): the final score row of each pass, the back-pointer
        rows L+1 .. R of each pass at their absolute times (every other row keeps bp_fill) and the FV_TV_* bits of
        the step-kernel instantiations that ran.  ob=None with T=...: on the rows staged by set_emissions."""
        ob, ptr, T = _ob_arg(ob, T)
        pa = (ForwardPass * len(passes))(*[ForwardPass(int(L), int(R), int(s)) for L, R, s in passes])
        rows = np.empty((len(passes), self.K), dtype=np.float32)
        bp = np.full((T, self.K), bp_fill, dtype=np.int32)
        variants = ctypes.c_ulonglong(0)
        self._check(self._L.fv_test_forward(self._h, ptr, T, pa, len(passes), _p(rows), _p(bp), ctypes.byref(variants)))
        return rows, bp, int(variants.value)

    def test_beam_forward(self, ob, beam, passes, T=None):
        """fv_test_beam_forward: passes = [(L, R, init_state, end_state)] run as one generation of FLASH-BS passes — the single
        whole-sequence pass (0, T-1, -1, -1) as generation 0 runs, anything else as a right-hand generation.  Returns a dict
        of the per-step buffers by absolute time, written in the passes' ranges only: scores[T, K] (rows outside: NaN),
        bp[T, K] (raw, TIE_TAG where a cell is still tagged; outside: -2), cut[T, 8], member_val / member_state[T, beam + 32],
        doubt[T, 1024], doubt_count[T], slot_val / slot_state[T, beam], path[T] (outside: -2), score, gate, variants, selects
        and rc (0, or WARN_BEAM_MISS).  ob=None with T=...: on the rows staged by set_emissions."""
        ob, ptr, T = _ob_arg(ob, T)
        K, BP = self.K, int(beam) + BEAM_EXTRA
        pa = (BeamPass * len(passes))(*[BeamPass(int(L), int(R), int(a), int(b)) for L, R, a, b in passes])
        o = dict(scores=np.full((T, K), np.nan, np.float32), bp=np.full((T, K), -2, np.int32),
                 cut=np.full((T, CUT_W), np.nan, np.float32), member_val=np.full((T, BP), np.nan, np.float32),
                 member_state=np.full((T, BP), -2, np.int32), doubt=np.full((T, DOUBT_CAP), -2, np.int32),
                 doubt_count=np.zeros(T, np.int32), slot_val=np.full((T, int(beam)), np.nan, np.float32),
                 slot_state=np.full((T, int(beam)), -2, np.int32), path=np.full(T, -2, np.int32),
                 score=np.full(1, np.nan, np.float32), gate=np.zeros(1, np.int32), variants=np.zeros(1, np.uint64),
                 selects=np.zeros(1, np.uint64))
        tab = BeamTables(**{k: _p(v).value for k, v in o.items()})
        rc = self._check(self._L.fv_test_beam_forward(self._h, ptr, T, int(beam), pa, len(passes), ctypes.byref(tab)))
        for k in ("gate", "variants", "selects"):
            o[k] = int(o[k][0])
        o["score"] = o["score"][0]
        o["rc"] = rc
        return o

    def test_beam_step(self, beam, sets, syms, speculative=False, theta=0.0, next_bound=float("inf"), cand_cap=0):
        """fv_test_beam_step: one launch of the beam step kernel over sets = [(values, states)] (beam <= n <= beam + 32),
        set q consuming symbol syms[q].  Returns a dict: scores[nsets, K] float32, bp[nsets, K] int32 (TIE_TAG-tagged
        where the maximum is tied), ties = set of (q, column), doubt = per set (count, list), cand = per set (count,
        list of (score, column)), variants."""
        K = self.K
        vals = [np.ascontiguousarray(v, dtype=np.float32) for v, _ in sets]
        sts = [np.ascontiguousarray(s, dtype=np.int32) for _, s in sets]
        arr = (BeamSet * len(sets))(*[BeamSet(_p(v).value, _p(s).value, v.size) for v, s in zip(vals, sts)])
        syms = np.ascontiguousarray(syms, dtype=np.int32)
        n = len(sets)
        scores = np.empty((n, K), dtype=np.float32)
        bp = np.empty((n, K), dtype=np.int32)
        ties = np.empty((n * K, 2), dtype=np.int32)
        nties = ctypes.c_int(0)
        doubt = np.empty((n, 1024), dtype=np.int32)
        doubt_counts = np.empty(n, dtype=np.int32)
        cand = np.empty((n, max(cand_cap, 1), 2), dtype=np.int32)
        cand_counts = np.zeros(n, dtype=np.int32)
        variants = ctypes.c_ulonglong(0)
        self._check(self._L.fv_test_beam_step(self._h, int(beam), arr, n, _p(syms), 1 if speculative else 0, float(theta),
                                              float(next_bound), int(cand_cap), _p(scores), _p(bp), _p(ties), ctypes.byref(nties),
                                              _p(doubt), _p(doubt_counts), _p(cand), _p(cand_counts), ctypes.byref(variants)))
        out_cand = []
        for q in range(n):
            c = int(cand_counts[q])
            rows = cand[q, :min(c, cand_cap)]
            out_cand.append((c, [(rows[i, 0:1].view(np.float32)[0], int(rows[i, 1])) for i in range(rows.shape[0])]))
        return dict(scores=scores, bp=bp, ties={(int(a), int(b)) for a, b in ties[:nties.value]},
                    doubt=[(int(doubt_counts[q]), doubt[q, :min(int(doubt_counts[q]), 1024)].tolist()) for q in range(n)],
                    cand=out_cand, variants=int(variants.value))

    def select_cand_cap(self, K, beam):
        """Capacity of the candidate list a decode's select has at (K, beam) under the current options (0: no lists)."""
        cap = ctypes.c_int(-1)
        self._check(self._L.fv_test_beam_select(self._h, int(K), int(beam), 0, None, 0, 0.0, 0.0, None, 0, ctypes.byref(cap),
                                                None, None, None, None, None, None, None))
        return int(cap.value)

    def test_beam_select(self, beam, rows, s=0, lists=None, prev_theta=0.0, prev_margin=0.0, seed=None, want_layout=True):
        """fv_test_beam_select: one select launch at lock-step s over rows[nsets, K] (K is the rows' width, not the
        model's; no model is needed).  lists: None, or per row None / (count, values, states) — a candidate list of `count`
        entries of which min(count, capacity) are given.  seed: None or (cut left here, cut left at the next time).
        Returns a dict: cut[nsets, 8] float32, members = per row (values, states) of the CUT_N entries in the order
        written, raw_val / raw_state[nsets, beam + 32] (NaN / -1 where nothing was written), counters = {index: total}
        for SELECT_COUNTERS, slot_val / slot_state[nsets, beam] (want_layout), selects = FV_TS_* bits, cand_cap."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, K = rows.shape
        BP = beam + BEAM_EXTRA
        keep = []
        arr = (SelectSet * n)()
        for q in range(n):
            arr[q].scores = rows[q:q + 1].ctypes.data
            if lists is not None and lists[q] is not None:
                count, vals, states = lists[q]
                rec = np.empty((len(vals), 2), dtype=np.int32)
                rec[:, 0] = np.ascontiguousarray(vals, dtype=np.float32).view(np.int32)
                rec[:, 1] = states
                keep.append(rec)
                arr[q].cand = rec.ctypes.data
                arr[q].cand_count = int(count)
        cap = ctypes.c_int(-1)
        cut = np.empty((n, CUT_W), dtype=np.float32)
        mval = np.empty((n, BP), dtype=np.float32)
        mstate = np.empty((n, BP), dtype=np.int32)
        counters = np.zeros(len(SELECT_COUNTERS), dtype=np.uint64)
        sval = np.empty((n, beam), dtype=np.float32)
        sstate = np.empty((n, beam), dtype=np.int32)
        selects = ctypes.c_ulonglong(0)
        sd = None if seed is None else np.ascontiguousarray(seed, dtype=np.float32)
        self._check(self._L.fv_test_beam_select(self._h, K, int(beam), int(s), arr, n, float(prev_theta), float(prev_margin),
                                                None if sd is None else _p(sd), 1 if want_layout else 0, ctypes.byref(cap),
                                                _p(cut), _p(mval), _p(mstate), _p(counters), _p(sval), _p(sstate),
                                                ctypes.byref(selects)))
        members = []
        for q in range(n):
            cn = int(cut[q, CUT_N]) if np.isfinite(cut[q, CUT_N]) else 0
            cn = max(0, min(cn, BP))
            members.append((mval[q, :cn].copy(), mstate[q, :cn].copy()))
        out = dict(cut=cut, members=members, raw_val=mval, raw_state=mstate,
                   counters={c: int(v) for c, v in zip(SELECT_COUNTERS, counters)}, selects=int(selects.value),
                   cand_cap=int(cap.value))
        if want_layout:
            out["slot_val"], out["slot_state"] = sval, sstate
        return out

    def stats(self):
        s = Stats()
        self._check(self._L.fv_last_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def set_partition(self, rank, nranks):
        self._check(self._L.fv_set_partition(self._h, rank, nranks))

    def comm_init(self, rank, nranks, unique_id):
        buf = ctypes.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        self._check(self._L.fv_comm_init(self._h, rank, nranks, buf))


def normalise_rows(counts):
    """The M-step of one table: every row of float64 counts divided by its sum; an all-zero row stays zero."""
    counts = np.asarray(counts, dtype=np.float64)
    total = counts.sum(axis=-1, keepdims=True)
    return np.divide(counts, total, out=np.zeros_like(counts), where=total > 0)


def baum_welch_step(fv, obs):
    """One EM iteration on the model fv holds: the E-step by fv.expected_counts(obs), the M-step on the host in float64
    (rows of trans and emit and the vector init normalised, all-zero rows left at zero), then fv.set_model with the float32
    result.  Returns the summed loglik of obs under the model it was called with."""
    c = fv.expected_counts(obs)
    fv.set_model(normalise_rows(c["trans"]).astype(np.float32), normalise_rows(c["emit"]).astype(np.float32),
                 normalise_rows(c["init"]).astype(np.float32))
    return float(np.sum(c["loglik"]))


def device_count():
    return int(load_library().fv_device_count())


def comm_unique_id():
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    rc = load_library().fv_comm_unique_id(buf)
    if rc != 0:
        raise FlashVitError(rc)
    return buf.raw
