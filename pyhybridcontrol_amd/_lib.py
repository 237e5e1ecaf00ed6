"""ctypes binding of libmldgpu.so (include/mldgpu.h).  No torch, no numpy compute: arrays in, arrays out.

The library is the product; there is no CPU fallback.  Importing this module never touches the GPU;
the first call that needs a device raises MldGpuError if none is present.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MLDGPU_LIB") or os.path.join(_HERE, "libmldgpu.so")      # (MLDGPU_LIB: a diagnostic build of the same library, scripts/ only)

MAT_NAMES = ("A", "B1", "B2", "B3", "B4", "b5", "C", "D1", "D2", "D3", "D4", "d5",
             "E", "F1", "F2", "F3", "F4", "f5", "G", "Psi")
EVO_NAMES = ("Phi_x", "Gamma_v", "Gamma_omega", "Gamma_5", "L_x", "L_v", "L_omega", "L_5",
             "H_x", "H_v", "H_omega", "H_5")
STATUS_NAMES = {0: "optimal", 1: "infeasible", 2: "node_limit", 3: "numerical", 4: "unbounded"}
COMM_ID_BYTES = 128
MLD_F32 = 1
MLD_SMALL_LDS = 2                      # mld_opts.flags: small problems in LDS, a wave per instance (k_small_milp)
MLD_DBG_SMALL_PIVOT_CAP = 1 << 25      # mld_opts.reserved: k_small_milp with a pivot budget of 2 (its declined instances go to the dense kernel)
MLD_DBG_PIVOT_SYNC_R5 = 1 << 26        # mld_opts.reserved: k_solve's pivot with its earlier barrier sequence (A/B on the same binary, bit-identical results)
MLD_DBG_SELECT_R6 = 1 << 27            # mld_opts.reserved: k_solve's choice of (row, column) with its earlier block reductions (A/B, bit-identical results)
MLD_DBG_UPDATE_R7 = 1 << 28            # mld_opts.reserved: k_solve's row updates as they were before a unit was cut down to its payload (A/B, bit-identical results)
MLD_DBG_DEAD_WORK_R8 = 1 << 29         # mld_opts.reserved: k_solve's bound changes update x_B of every row, unmaintained ones included, as before (A/B, bit-identical results)
MLD_SIM_ADVANCE, MLD_SIM_ACTUAL, MLD_SIM_LOG = 1, 2, 4      # flags of mld_sim_step_batch / mld_sim_step_resolve
MLD_START_KEEP = 1                                          # flags of mld_warm_start_from_rollout: instances that already have a start keep it
MLD_ROLLOUT_COMPLETE_DEVICE, MLD_ROLLOUT_COMPLETE_DBG_FIRST_ONLY = 1, 2      # mode of mld_set_rollout_completion (the second: tests only)
MLD_FB_MEMORY, MLD_FB_POLICY = 1, 2                         # fb of mld_sim_step_fallback: the sources an instance without a usable plan may take its u from


class MldGpuError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("nx", "nu", "ndelta", "nz", "nmu", "nomega", "ny", "nc", "nu_l", "nmu_l")]


class Opts(C.Structure):
    _fields_ = [("gap_abs", C.c_double), ("gap_rel", C.c_double), ("max_nodes", C.c_int32),
                ("max_pivots", C.c_int32), ("cut_rounds", C.c_int32), ("cuts_per_round", C.c_int32),
                ("max_cuts", C.c_int32), ("presolve", C.c_int32), ("n_slots", C.c_int32), ("mir_per_round", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32), ("time_limit", C.c_double)]


class Cost(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("lin_v", "lin_x", "lin_y", "quad_v", "quad_x", "quad_y")]


class Stats(C.Structure):
    _fields_ = [("nodes", C.c_int64), ("pivots", C.c_int64), ("cuts", C.c_int64), ("refactors", C.c_int64),
                ("n_optimal", C.c_int32), ("n_infeasible", C.c_int32), ("n_node_limit", C.c_int32),
                ("n_numerical", C.c_int32), ("solve_ms", C.c_double), ("rhs_ms", C.c_double)]


_lib = None

# every symbol include/mldgpu.h declares (tests check that the shared object exports all of them)
EXPORTS = ("mld_device_count", "mld_set_device", "mld_last_error", "mld_version", "mld_device_info",
           "mld_opts_size", "mld_model_create", "mld_model_create_tv", "mld_model_destroy", "mld_condense_device", "mld_condense", "mld_condense_device_f32", "mld_condense_f32", "mld_opts_default",
           "mld_problem_create", "mld_problem_set_cost", "mld_problem_destroy", "mld_cost_assemble",
           "mld_solve_batch", "mld_upload_batch", "mld_upload_constraint_blocks", "mld_upload_constraint_blocks_x", "mld_solve_resident", "mld_problem_use_stream", "mld_solve_launch", "mld_solve_finish", "mld_download_results", "mld_download_telemetry",
           "mld_rhs_batch", "mld_problem_set_opts", "mld_problem_get_opts", "mld_advance_batch", "mld_advance_batch2", "mld_set_warm_start", "mld_warm_start_from_previous", "mld_set_cutoffs", "mld_record_open_nodes", "mld_download_open_nodes", "mld_set_handoff", "mld_handoff_stats", "mld_small_lds_stats", "mld_set_handoff_policy", "mld_set_std_block", "mld_download_inputs", "mld_stage_inputs", "mld_select_inputs", "mld_upload_instance_cost", "mld_download_instance_cost", "mld_predict_batch", "mld_evaluate_batch", "mld_gather_results",
           "mld_upload_profiles", "mld_forecast_from_profiles", "mld_constraint_blocks_from_profiles", "mld_evaluate_batch_profiles", "mld_download_constraint_blocks",
           "mld_sim_log_begin", "mld_sim_log_count", "mld_sim_step_batch", "mld_download_sim_log",
           "mld_sim_step_resolve", "mld_download_sim_log_aux", "mld_rollout_batch",
           "mld_upload_policy", "mld_set_policy_state", "mld_download_policy_state", "mld_rollout_policy", "mld_sim_step_policy",
           "mld_plan_memory", "mld_set_plan_memory", "mld_download_plan_memory", "mld_sim_step_fallback", "mld_download_sim_log_source",
           "mld_upload_prices", "mld_set_price_cost", "mld_instance_cost_from_prices", "mld_set_stage_cost", "mld_sim_log_cost_begin", "mld_download_sim_log_cost",
           "mld_download_cost_total", "mld_sim_log_summary", "mld_rollout_kpi", "mld_rollout_risk", "mld_rollout_select", "mld_rollout_select_policy",
           "mld_warm_start_from_rollout", "mld_set_rollout_completion", "mld_rollout_completion_stats",
           "mld_keep_selection", "mld_set_selection", "mld_download_selection", "mld_sim_step_selected", "mld_download_sim_log_pick",
           "mld_comm_unique_id", "mld_comm_init", "mld_gather", "mld_comm_destroy")


def load():
    """dlopen the in-tree library (built by pyhybridcontrol_amd.build); raises if it is missing"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MldGpuError("libmldgpu.so is not built (run `python -m pyhybridcontrol_amd.build`); "
                          "there is no CPU fallback for the MPC solve path")
    lib = C.CDLL(LIB_PATH)
    lib.mld_last_error.restype = C.c_char_p
    lib.mld_version.restype = C.c_char_p
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("mld_last_error", "mld_version"):
            fn.restype = C.c_int
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.mld_evaluate_batch.argtypes = [C.c_void_p, dp, C.c_int, dp, ip, dp, dp, dp, ip, dp, dp]
    lp = C.POINTER(C.c_int64)
    lib.mld_upload_profiles.argtypes = [C.c_void_p, C.c_int64, dp, C.c_int, ip]
    lib.mld_forecast_from_profiles.argtypes = [C.c_void_p, lp, C.c_int]
    lib.mld_constraint_blocks_from_profiles.argtypes = [C.c_void_p, C.c_int, lp, C.c_int, ip, dp]
    lib.mld_evaluate_batch_profiles.argtypes = [C.c_void_p, dp, C.c_int, lp, C.c_int, ip, dp, dp, dp, ip, dp, dp]
    lib.mld_download_constraint_blocks.argtypes = [C.c_void_p, ip, dp, ip, dp]
    bp = C.POINTER(C.c_uint8)
    lib.mld_sim_log_begin.argtypes = [C.c_void_p, C.c_int]
    lib.mld_sim_log_count.argtypes = [C.c_void_p, ip, ip]
    lib.mld_sim_step_batch.argtypes = [C.c_void_p, dp, lp, C.c_int, C.c_int, dp, dp, bp, dp, ip, ip]
    lib.mld_download_sim_log.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, dp, dp, dp, bp, dp, ip, dp, dp, ip, ip]
    lib.mld_sim_step_resolve.argtypes = [C.c_void_p, C.c_void_p, dp, lp, C.c_int, C.c_int, dp, dp, bp, dp, ip, dp, ip, ip]
    lib.mld_download_sim_log_aux.argtypes = [C.c_void_p, C.c_int, C.c_int, ip]
    lib.mld_rollout_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, dp, dp, lp, C.c_int, dp, C.c_int, dp, dp, dp, dp, ip, dp, dp, dp, ip, ip, ip, lp]
    lib.mld_upload_policy.argtypes = [C.c_void_p, dp, dp, dp, dp, dp, ip]
    lib.mld_set_policy_state.argtypes = [C.c_void_p, dp]
    lib.mld_download_policy_state.argtypes = [C.c_void_p, dp]
    lib.mld_rollout_policy.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, dp, dp, dp, lp, C.c_int, dp, C.c_int, dp, dp, dp, dp, ip, dp, dp, dp, ip, ip, ip, ip, lp]
    lib.mld_sim_step_policy.argtypes = list(lib.mld_sim_step_resolve.argtypes)
    lib.mld_plan_memory.argtypes = [C.c_void_p, C.c_int]
    lib.mld_set_plan_memory.argtypes = [C.c_void_p, dp, ip]
    lib.mld_download_plan_memory.argtypes = [C.c_void_p, dp, ip]
    lib.mld_sim_step_fallback.argtypes = [C.c_void_p, C.c_void_p, C.c_int, lp, C.c_int, C.c_int, dp, dp, bp, dp, ip, dp, ip, ip, ip]
    lib.mld_download_sim_log_source.argtypes = [C.c_void_p, C.c_int, C.c_int, ip]
    lib.mld_upload_prices.argtypes = [C.c_void_p, C.c_int64, dp, C.c_int]
    lib.mld_set_price_cost.argtypes = [C.c_void_p, dp, dp, dp]
    lib.mld_instance_cost_from_prices.argtypes = [C.c_void_p, lp, C.c_int]
    lib.mld_set_stage_cost.argtypes = [C.c_void_p, dp, dp]
    lib.mld_sim_log_cost_begin.argtypes = [C.c_void_p, lp]
    lib.mld_download_sim_log_cost.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp]
    lib.mld_download_cost_total.argtypes = [C.c_void_p, dp, ip]
    lib.mld_sim_log_summary.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, ip, dp, C.c_double,
                                        dp, dp, dp, ip, ip, ip, ip, ip, dp, ip, ip, lp, ip]
    lib.mld_rollout_kpi.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp, dp, lp, C.c_int, dp, C.c_int, C.c_int, dp, dp, dp, dp, dp, ip, dp, C.c_double, lp,
                                    dp, dp, dp, dp, ip, dp, dp, dp, ip, ip, ip, ip, lp, dp, dp, dp, ip, ip, ip, ip, ip]
    lib.mld_rollout_risk.argtypes = list(lib.mld_rollout_kpi.argtypes) + [C.c_int, ip, ip, dp, C.c_int, dp, dp, dp, dp, ip, ip, ip, dp, ip, dp, dp, ip]
    lib.mld_rollout_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, lp, C.c_int, dp, C.c_int, C.c_int, dp, dp, dp, dp, dp, ip, dp, C.c_double, lp,
                                       C.c_int, ip, ip, dp, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, ip, dp, C.c_int,
                                       ip, dp, ip, bp, dp, dp, dp, dp, dp, ip, ip, ip, dp, ip, dp, dp, ip,
                                       dp, dp, dp, ip, ip, ip, lp, dp, dp, dp, ip, ip, ip, ip, ip]
    lib.mld_rollout_select_policy.argtypes = list(lib.mld_rollout_select.argtypes) + [C.c_int, dp, dp, dp, dp, dp, ip, dp, ip]
    lib.mld_warm_start_from_rollout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, dp, dp, C.c_int, ip, lp]
    lib.mld_set_rollout_completion.argtypes = [C.c_void_p, C.c_int]
    lib.mld_rollout_completion_stats.argtypes = [C.c_void_p, lp]
    lib.mld_keep_selection.argtypes = [C.c_void_p, C.c_int]
    lib.mld_set_selection.argtypes = [C.c_void_p, C.c_int, ip, ip, dp]
    lib.mld_download_selection.argtypes = [C.c_void_p, ip, ip, ip, dp, ip]
    lib.mld_sim_step_selected.argtypes = list(lib.mld_sim_step_fallback.argtypes) + [ip]
    lib.mld_download_sim_log_pick.argtypes = [C.c_void_p, C.c_int, C.c_int, ip]
    if int(lib.mld_opts_size()) != C.sizeof(Opts):
        raise MldGpuError("libmldgpu.so was built with another layout of mld_opts (%d bytes, this binding %d): rebuild it (python -m pyhybridcontrol_amd.build)"
                          % (lib.mld_opts_size(), C.sizeof(Opts)))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise MldGpuError("libmldgpu error %d: %s" % (rc, load().mld_last_error().decode()))


def device_count():
    return int(load().mld_device_count())


def version():
    return load().mld_version().decode()


def device_info():
    name = C.create_string_buffer(64)
    ncu, hbm, lds = C.c_int(), C.c_int64(), C.c_int()
    check(load().mld_device_info(name, 64, C.byref(ncu), C.byref(hbm), C.byref(lds)))
    return dict(name=name.value.decode(), n_cu=ncu.value, hbm_bytes=hbm.value, lds_bytes=lds.value)


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a
