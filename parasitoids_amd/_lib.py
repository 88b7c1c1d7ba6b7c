"""ctypes binding of libparasitoid_hip.so (C ABI: include/parasitoid_hip.h).

Importing this module does not touch the GPU (fork-safe, like the reference's
lazy `import cuda_lib`, CalcSol.py:162).  `load()` raises ImportError when the
shared library is missing; there is no CPU fallback in this package.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libparasitoid_hip.so')

PS_OK = 0
PS_ERR_NO_DEVICE = -1
PS_ERR_OOM = -2
PS_ERR_BAD_SHAPE = -3
PS_ERR_BAD_ARG = -4
PS_ERR_UNSUPPORTED = -5
PS_ERR_HIP = -6
PS_ERR_HPROB_BOUNDS = -7
PS_ERR_PMF_NEGATIVE = -8
PS_ERR_FLIGHT_PROB = -9
PS_ERR_STATE = -10
PS_ERR_EMPTY = -11

MODE_EXACT = 0
MODE_FAST = 1
MODE_FOLD = 2
MODE_AUTO = 3

REC_CHAIN, REC_BACK, REC_STATE, REC_WSUM = 0, 1, 2, 3
REC_NONE = -1       # ps_sites_apply only: the group is not released yet on that output day


class DayStats(C.Structure):
    _fields_ = [('nnz', C.c_int64), ('sum', C.c_double), ('delta', C.c_double),
                ('padmax', C.c_double), ('flag', C.c_int32), ('pad_', C.c_int32)]


class HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('libparasitoid_hip error %d: %s' % (code, msg))
        self.code = code


_I32P = C.POINTER(C.c_int32)
_I64P = C.POINTER(C.c_int64)
_F64P = C.POINTER(C.c_double)
_VP = C.c_void_p

# name -> (restype, argtypes); every symbol include/parasitoid_hip.h declares
SIGNATURES = {
    'ps_version': (C.c_int, []),
    'ps_device_count': (C.c_int, []),
    'ps_last_error': (C.c_char_p, []),
    'ps_device_info': (C.c_int, [C.c_int, C.c_char_p, C.c_int, _I32P, _I64P]),
    'ps_row_live_units': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _I32P, _I32P, _I32P, C.c_int]),
    'ps_row_fwd_info': (C.c_int, [C.c_int, _I32P, _I32P]),
    'ps_row_fwd_stage_info': (C.c_int, [C.c_int, C.c_int, _I32P]),
    'ps_row_fwd_stage_lds': (C.c_int64, [C.c_int, C.c_int]),
    'ps_row_fwd_stage_bytes': (C.c_int64, [C.c_int, C.c_int]),
    'ps_row_fwd_stage_slot': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'ps_row_fwd_stage_walk': (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, _I64P]),
    'ps_solver_create': (C.c_int, [C.POINTER(_VP), C.c_int, C.c_int, C.c_int, C.c_int]),
    'ps_solver_destroy': (C.c_int, [_VP]),
    'ps_solver_info': (C.c_int, [_VP, _I32P, _I32P, _I32P, _I32P]),
    'ps_solver_sync': (C.c_int, [_VP]),
    'ps_solver_set_option': (C.c_int, [_VP, C.c_char_p, C.c_double]),
    'ps_solver_get_option': (C.c_int, [_VP, C.c_char_p, _F64P]),
    'ps_solver_set_state_coo': (C.c_int, [_VP, _I32P, _I32P, _F64P, C.c_int64]),
    'ps_solver_fftconv2_coo': (C.c_int, [_VP, _I32P, _I32P, _F64P, C.c_int64, C.c_int]),
    'ps_solver_get_cursol': (C.c_int, [_VP, C.c_double, C.c_double, C.c_int, C.POINTER(DayStats)]),
    'ps_solver_back_solve': (C.c_int, [_VP, C.c_int, _I64P, _I32P, _I32P, _F64P, C.c_double,
                                       C.c_double, C.POINTER(DayStats)]),
    'ps_chain_set_kernels': (C.c_int, [_VP, C.c_int, _I64P, _I32P, _I32P, _I32P, _F64P]),
    'ps_chain_run': (C.c_int, [_VP, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]),
    'ps_chain_stats': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(DayStats)]),
    'ps_chain_run_release': (C.c_int, [_VP, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _F64P,
                                       C.POINTER(C.c_int)]),
    'ps_record_stats': (C.c_int, [_VP, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                  C.POINTER(DayStats)]),
    'ps_solver_retarget': (C.c_int, [_VP, C.c_int]),
    'ps_fast_size': (C.c_int, [C.c_int, C.c_int]),
    'ps_solver_kernels_direct': (C.c_int, [_VP]),
    'ps_solver_pipeline': (C.c_int, [_VP]),
    'ps_solver_deferred_info': (C.c_int, [_VP, _I32P, _I64P]),
    'ps_solver_auto_info': (C.c_int, [_VP, _I32P, _I32P]),
    'ps_solver_auto_route': (C.c_int, [_VP, C.c_int, C.c_int, _I32P]),
    'ps_record_fetch_coo': (C.c_int, [_VP, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                      C.c_double, _I32P, _I32P, _F64P, C.c_int64, _I64P]),
    'ps_record_fetch_csr': (C.c_int, [_VP, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                      C.c_double, _I32P, _I32P, _F64P, C.c_int64, _I64P]),
    'ps_record_fetch_dense': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_record_gather': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int64, _I32P, _I32P, C.c_double,
                                   C.c_double, _F64P]),
    'ps_record_gather_multi': (C.c_int, [_VP, C.c_int, _I32P, _I32P, C.c_int64, _I32P, _I32P, C.c_double,
                                          C.c_double, _F64P]),
    'ps_weighted_sum': (C.c_int, [_VP, C.c_int, _I32P, _I32P, _F64P]),
    'ps_prof_enable': (C.c_int, [_VP, C.c_int]),
    'ps_prof_read': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_prof_read_days': (C.c_int, [_VP, C.c_int, _I64P]),
    'ps_prof_read_launches': (C.c_int, [_VP, C.c_int, _I64P]),
    'ps_chain_block_prefix': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    'ps_chain_block_finish': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_double, C.c_double,
                                        C.c_int, C.POINTER(C.c_int)]),
    'ps_device_copy': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'ps_prof_read_owner': (C.c_int, [_VP, C.c_int, C.c_int, _F64P, _I64P, _I64P, _I64P]),
    'ps_solver_owner_fft': (C.c_int, [_VP, C.c_int]),
    'ps_solver_get_spectrum': (C.c_int, [_VP, _F64P]),
    'ps_solver_set_spectrum': (C.c_int, [_VP, _F64P]),
    'ps_model_create': (C.c_int, [C.POINTER(_VP), C.c_int]),
    'ps_model_destroy': (C.c_int, [_VP]),
    'ps_model_set_option': (C.c_int, [_VP, C.c_char_p, C.c_double]),
    'ps_model_set_wind': (C.c_int, [_VP, _F64P, _I32P, C.c_int, C.c_int, C.c_int]),
    'ps_model_prob_mass': (C.c_int, [_VP, C.c_int, _I32P, _F64P, _F64P, _F64P, _F64P, C.c_double,
                                     C.c_int, C.c_double, C.c_int, _I32P, _I64P, _I32P, _I32P]),
    'ps_model_fetch_coo': (C.c_int, [_VP, C.c_int, _I32P, _I32P, _F64P, C.c_int64]),
    'ps_model_fetch_debug': (C.c_int, [_VP, C.c_int, _F64P, _I32P, _F64P, _F64P]),
    'ps_model_hflight': (C.c_int, [_VP, C.c_int, _F64P, _F64P]),
    'ps_model_mvn_cdf_values': (C.c_int, [_VP, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_double, C.c_double, _I32P, _F64P, C.c_int64]),
    'ps_chain_set_kernels_from_model': (C.c_int, [_VP, _VP, C.c_int, C.c_int]),
    'ps_chain_set_kernels_from_model_indexed': (C.c_int, [_VP, _VP, _I32P, C.c_int]),
    'ps_solver_set_state_from_model': (C.c_int, [_VP, _VP, C.c_int]),
    'ps_model_export_device': (C.c_int, [_VP, C.c_int, C.c_int, _VP, _VP, _VP, C.c_int64]),
    'ps_chain_set_kernels_device': (C.c_int, [_VP, C.c_int, _I64P, _I32P, _VP, _VP, _VP]),
    'ps_solver_set_state_device': (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, C.c_int]),
    'ps_summary_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_summary_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double,
                                 C.c_uint32]),
    'ps_summary_merge': (C.c_int, [_VP, _VP]),
    'ps_summary_info': (C.c_int, [_VP, _F64P, _I64P]),
    'ps_summary_fetch': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_summary_reset': (C.c_int, [_VP]),
    'ps_summary_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_summary_destroy': (None, [_VP]),
    'ps_linspread_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_linspread_set_center': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_linspread_add': (C.c_int, [_VP, _VP, C.c_int, C.c_double, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P,
                                   C.c_double]),
    'ps_linspread_finalize': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_linspread_fetch': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_linspread_info': (C.c_int, [_VP, _I32P, _I32P, _I64P]),
    'ps_linspread_reset': (C.c_int, [_VP]),
    'ps_linspread_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_linspread_destroy': (None, [_VP]),
    'ps_hist_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_hist_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_hist_merge': (C.c_int, [_VP, _VP]),
    'ps_hist_info': (C.c_int, [_VP, _F64P, _I64P, _I32P]),
    'ps_hist_quantile': (C.c_int, [_VP, C.c_int, C.c_double, _F64P, _F64P, _F64P]),
    'ps_hist_exceed': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_hist_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_hist_reset': (C.c_int, [_VP]),
    'ps_hist_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_hist_destroy': (None, [_VP]),
    'ps_arrival_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_arrival_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_arrival_merge': (C.c_int, [_VP, _VP]),
    'ps_arrival_info': (C.c_int, [_VP, _F64P, _I64P]),
    'ps_arrival_prob': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_arrival_quantile': (C.c_int, [_VP, C.c_int, C.c_double, _I32P]),
    'ps_arrival_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_arrival_fetch_reached': (C.c_int, [_VP, C.c_int64, C.c_int64, C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32)]),
    'ps_arrival_reset': (C.c_int, [_VP]),
    'ps_arrival_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_arrival_destroy': (None, [_VP]),
    'ps_project_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_project_apply': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_project_fetch': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_project_gather': (C.c_int, [_VP, C.c_int64, _I32P, _I32P, _F64P]),
    'ps_project_info': (C.c_int, [_VP, _I32P, _I32P, _I32P, _I64P]),
    'ps_project_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_project_destroy': (None, [_VP]),
    'ps_summary_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_hist_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_arrival_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_sites_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _I32P, _I32P, _I32P, _F64P, C.POINTER(_VP)]),
    'ps_sites_apply': (C.c_int, [_VP, _VP, C.c_int, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_sites_fetch': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_sites_gather': (C.c_int, [_VP, C.c_int64, _I32P, _I32P, _F64P]),
    'ps_sites_info': (C.c_int, [_VP, _I32P, _I32P, _I32P, _I32P, _I64P]),
    'ps_sites_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_sites_destroy': (None, [_VP]),
    'ps_summary_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_hist_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_arrival_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_sens_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    'ps_sens_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_int, _F64P,
                              C.c_uint32]),
    'ps_sens_add_project': (C.c_int, [_VP, _VP, C.c_int, _F64P, C.c_uint32]),
    'ps_sens_add_sites': (C.c_int, [_VP, _VP, C.c_int, _F64P, C.c_uint32]),
    'ps_sens_merge': (C.c_int, [_VP, _VP, C.c_int, _F64P]),
    'ps_sens_finalize': (C.c_int, [_VP, C.c_int, C.c_int, _F64P, _F64P]),
    'ps_sens_fetch': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_sens_info': (C.c_int, [_VP, _F64P, _I64P]),
    'ps_sens_reset': (C.c_int, [_VP]),
    'ps_sens_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_sens_destroy': (None, [_VP]),
    'ps_depend_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    'ps_depend_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_int, _I32P,
                                C.c_uint32]),
    'ps_depend_add_project': (C.c_int, [_VP, _VP, C.c_int, _I32P, C.c_uint32]),
    'ps_depend_add_sites': (C.c_int, [_VP, _VP, C.c_int, _I32P, C.c_uint32]),
    'ps_depend_merge': (C.c_int, [_VP, _VP]),
    'ps_depend_finalize': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_depend_fetch': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_depend_info': (C.c_int, [_VP, _F64P, _I64P]),
    'ps_depend_reset': (C.c_int, [_VP]),
    'ps_depend_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_depend_destroy': (None, [_VP]),
    'ps_contrast_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_contrast_add_sites': (C.c_int, [_VP, _VP, _VP, C.c_uint32]),
    'ps_contrast_add_project': (C.c_int, [_VP, _VP, _VP, C.c_uint32]),
    'ps_contrast_merge': (C.c_int, [_VP, _VP]),
    'ps_contrast_info': (C.c_int, [_VP, _F64P, _I64P]),
    'ps_contrast_fetch': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_contrast_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_contrast_fetch_coverage': (C.c_int, [_VP, C.c_int64, C.c_int64, C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32)]),
    'ps_contrast_reset': (C.c_int, [_VP]),
    'ps_contrast_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_contrast_destroy': (None, [_VP]),
    'ps_rank_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_rank_add_sites': (C.c_int, [_VP, C.POINTER(_VP), C.c_int, C.c_uint32]),
    'ps_rank_add_project': (C.c_int, [_VP, C.POINTER(_VP), C.c_int, C.c_uint32]),
    'ps_rank_merge': (C.c_int, [_VP, _VP]),
    'ps_rank_info': (C.c_int, [_VP, _F64P, _I64P]),
    'ps_rank_fetch': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_rank_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_rank_fetch_coverage': (C.c_int, [_VP, C.c_int64, C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    'ps_rank_reset': (C.c_int, [_VP]),
    'ps_rank_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_rank_destroy': (None, [_VP]),
    'ps_mcerr_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.c_uint32, C.POINTER(_VP)]),
    'ps_mcerr_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_mcerr_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_mcerr_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_mcerr_finish': (C.c_int, [_VP]),
    'ps_mcerr_merge': (C.c_int, [_VP, _VP]),
    'ps_mcerr_info': (C.c_int, [_VP, _I64P, _I64P, _I64P, _I64P, _I64P, _I64P]),
    'ps_mcerr_fetch': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_mcerr_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    'ps_mcerr_rhat': (C.c_int, [C.POINTER(_VP), C.c_int, C.c_int, _F64P]),
    'ps_mcerr_reset': (C.c_int, [_VP]),
    'ps_mcerr_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_mcerr_destroy': (None, [_VP]),
    'ps_nested_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    'ps_nested_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_nested_add_project': (C.c_int, [_VP, _VP]),
    'ps_nested_add_sites': (C.c_int, [_VP, _VP]),
    'ps_nested_close': (C.c_int, [_VP, C.c_uint32]),
    'ps_nested_merge': (C.c_int, [_VP, _VP]),
    'ps_nested_finalize': (C.c_int, [_VP]),
    'ps_nested_info': (C.c_int, [_VP, _F64P, _I64P, _I64P, _I64P, _F64P]),
    'ps_nested_fetch': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_nested_reset': (C.c_int, [_VP]),
    'ps_nested_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_nested_destroy': (None, [_VP]),
    'ps_peak_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_peak_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_peak_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_peak_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_peak_merge': (C.c_int, [_VP, _VP]),
    'ps_peak_info': (C.c_int, [_VP, _F64P, _I64P]),
    'ps_peak_reset': (C.c_int, [_VP]),
    'ps_peak_fetch_field': (C.c_int, [_VP, _F64P]),
    'ps_peak_fetch_day_counts': (C.c_int, [_VP, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_peak_fetch_duration_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_peak_day_prob': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_peak_day_quantile': (C.c_int, [_VP, C.c_double, _I32P]),
    'ps_peak_duration_prob': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_peak_duration_quantile': (C.c_int, [_VP, C.c_int, C.c_double, _I32P]),
    'ps_peak_duration_mean': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_peak_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_peak_destroy': (None, [_VP]),
    'ps_summary_add_peak': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_hist_add_peak': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_excur_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_excur_reserve': (C.c_int, [_VP, C.c_int64]),
    'ps_excur_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_excur_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_excur_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_excur_add_peak': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_excur_merge': (C.c_int, [_VP, _VP]),
    'ps_excur_info': (C.c_int, [_VP, _F64P, _I64P, _I64P, _I64P]),
    'ps_excur_reset': (C.c_int, [_VP]),
    'ps_excur_finalize': (C.c_int, [_VP]),
    'ps_excur_map': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_excur_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_excur_fetch_mask': (C.c_int, [_VP, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    'ps_excur_fetch_bounds': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32)]),
    'ps_excur_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_excur_destroy': (None, [_VP]),
    'ps_wsum_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_wsum_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_int, _F64P,
                              _F64P]),
    'ps_wsum_add_project': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_wsum_add_sites': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_wsum_add_peak': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_wsum_merge': (C.c_int, [_VP, _VP, _F64P, _F64P]),
    'ps_wsum_info': (C.c_int, [_VP, _F64P, _I64P, _I64P]),
    'ps_wsum_fetch': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_wsum_reset': (C.c_int, [_VP]),
    'ps_wsum_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_wsum_destroy': (None, [_VP]),
    'ps_whist_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_whist_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_int, _F64P,
                               _F64P]),
    'ps_whist_add_project': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_whist_add_sites': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_whist_merge': (C.c_int, [_VP, _VP, _F64P, _F64P]),
    'ps_whist_info': (C.c_int, [_VP, _F64P, _I64P, _I64P]),
    'ps_whist_quantile': (C.c_int, [_VP, C.c_int, C.c_int, C.c_double, _F64P, _F64P, _F64P, _I32P]),
    'ps_whist_exceed': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_whist_fetch': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_whist_reset': (C.c_int, [_VP]),
    'ps_whist_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P, _F64P, _I64P]),
    'ps_whist_destroy': (None, [_VP]),
    'ps_warr_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_warr_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_int, _F64P,
                              _F64P]),
    'ps_warr_add_project': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_warr_add_sites': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_warr_merge': (C.c_int, [_VP, _VP, _F64P, _F64P]),
    'ps_warr_info': (C.c_int, [_VP, _F64P, _I64P, _I64P]),
    'ps_warr_prob': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_warr_quantile': (C.c_int, [_VP, C.c_int, C.c_int, C.c_double, _I32P]),
    'ps_warr_fetch': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_warr_reset': (C.c_int, [_VP]),
    'ps_warr_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P, _F64P, _I64P]),
    'ps_warr_destroy': (None, [_VP]),
    'ps_catch_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _I32P, _F64P, _I32P, C.POINTER(_VP)]),
    'ps_catch_apply': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_catch_apply_project': (C.c_int, [_VP, _VP]),
    'ps_catch_apply_sites': (C.c_int, [_VP, _VP]),
    'ps_catch_fetch': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_catch_gather': (C.c_int, [_VP, C.c_int64, _I32P, _I32P, _F64P]),
    'ps_catch_info': (C.c_int, [_VP, _I32P, _I32P, _I32P, _I64P]),
    'ps_catch_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_catch_destroy': (None, [_VP]),
    'ps_summary_add_catch': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_mcerr_add_catch': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_wsum_add_catch': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_nbhd_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _I32P, _I32P, C.POINTER(_VP)]),
    'ps_nbhd_set_skip': (C.c_int, [_VP, C.c_int]),
    'ps_nbhd_apply': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_nbhd_apply_project': (C.c_int, [_VP, _VP]),
    'ps_nbhd_apply_sites': (C.c_int, [_VP, _VP]),
    'ps_nbhd_fetch': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_nbhd_gather': (C.c_int, [_VP, C.c_int64, _I32P, _I32P, _F64P]),
    'ps_nbhd_info': (C.c_int, [_VP, _I32P, _I32P, _I32P, _I64P]),
    'ps_nbhd_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_nbhd_destroy': (None, [_VP]),
    'ps_summary_add_nbhd': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_hist_add_nbhd': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_mcerr_add_nbhd': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_wsum_add_nbhd': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_prox_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _I32P, _F64P, _I32P, C.c_double, C.POINTER(_VP)]),
    'ps_prox_set_strip': (C.c_int, [_VP, C.c_int]),
    'ps_prox_apply': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_prox_apply_project': (C.c_int, [_VP, _VP]),
    'ps_prox_apply_sites': (C.c_int, [_VP, _VP]),
    'ps_prox_fetch': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_prox_fetch_d2': (C.c_int, [_VP, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_prox_gather': (C.c_int, [_VP, C.c_int64, _I32P, _I32P, _F64P]),
    'ps_prox_info': (C.c_int, [_VP, _I32P, _I32P, _I32P, _I64P, _I32P]),
    'ps_prox_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_prox_destroy': (None, [_VP]),
    'ps_origin_create': (C.c_int, [C.c_int, C.c_int, C.c_int, _I32P, _I32P, _I32P, _I32P, _F64P, _F64P, C.c_int, C.c_int,
                                   _F64P, _I32P, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_origin_reserve': (C.c_int, [_VP, C.c_int64]),
    'ps_origin_add': (C.c_int, [_VP, _VP, C.c_int, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_origin_merge': (C.c_int, [_VP, _VP]),
    'ps_origin_reset': (C.c_int, [_VP]),
    'ps_origin_fetch': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_origin_members': (C.c_int, [_VP, C.c_int64, _F64P, C.POINTER(C.c_uint32)]),
    'ps_origin_info': (C.c_int, [_VP, _F64P, _I64P, _I64P, _I64P]),
    'ps_origin_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P, _F64P, _I64P]),
    'ps_origin_destroy': (None, [_VP]),
    'ps_origin_set_known': (C.c_int, [_VP, C.c_int, _I32P, _I32P, _F64P, _I32P, C.c_int]),
    'ps_origin_background': (C.c_int, [_VP, _VP, C.c_int, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_origin_fetch_background': (C.c_int, [_VP, _F64P, _F64P]),
    'ps_origin_null_rows': (C.c_int, [_VP, C.c_int64, _F64P]),
    'ps_summary_add_prox': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_hist_add_prox': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_mcerr_add_prox': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_wsum_add_prox': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_gain_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _I32P, _F64P, _I32P, C.POINTER(_VP)]),
    'ps_gain_apply': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double]),
    'ps_gain_apply_project': (C.c_int, [_VP, _VP]),
    'ps_gain_apply_sites': (C.c_int, [_VP, _VP]),
    'ps_summary_add_gain': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_wsum_add_gain': (C.c_int, [_VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_gain_finish_summary': (C.c_int, [_VP, _VP]),
    'ps_gain_finish_wsum': (C.c_int, [_VP, _VP, C.c_int]),
    'ps_gain_fetch': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_gain_fetch_result': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_gain_gather': (C.c_int, [_VP, C.c_int64, _I32P, _I32P, _F64P]),
    'ps_gain_info': (C.c_int, [_VP, _I32P, _I32P, _I32P, _I32P, _I64P]),
    'ps_gain_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_gain_destroy': (None, [_VP]),
    'ps_range_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_range_reserve': (C.c_int, [_VP, C.c_int64]),
    'ps_range_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_range_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_range_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_range_merge': (C.c_int, [_VP, _VP]),
    'ps_range_info': (C.c_int, [_VP, _F64P, _I64P, _I64P, _I64P]),
    'ps_range_reset': (C.c_int, [_VP]),
    'ps_range_prob': (C.c_int, [_VP, C.c_int, C.c_int, _F64P]),
    'ps_range_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_range_fetch_members': (C.c_int, [_VP, C.c_int, C.c_int, _F64P, C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32)]),
    'ps_range_fetch_mass': (C.c_int, [_VP, C.c_int, C.POINTER(C.c_uint64), _I32P]),
    'ps_range_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_range_destroy': (None, [_VP]),
    'ps_patch_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.c_int, C.POINTER(_VP)]),
    'ps_patch_reserve': (C.c_int, [_VP, C.c_int64]),
    'ps_patch_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_patch_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_patch_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_patch_merge': (C.c_int, [_VP, _VP]),
    'ps_patch_info': (C.c_int, [_VP, _F64P, _I64P, _I64P, _I64P]),
    'ps_patch_reset': (C.c_int, [_VP]),
    'ps_patch_prob': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_patch_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_patch_fetch_members': (C.c_int, [_VP, C.c_int, C.c_int] + [C.POINTER(C.c_uint32)] * 6),
    'ps_patch_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_patch_destroy': (None, [_VP]),
    'ps_pathway_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.c_int, C.c_int, _I32P, _I32P,
                                    C.POINTER(_VP)]),
    'ps_pathway_reserve': (C.c_int, [_VP, C.c_int64]),
    'ps_pathway_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_pathway_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_pathway_merge': (C.c_int, [_VP, _VP]),
    'ps_pathway_info': (C.c_int, [_VP, _F64P, _I64P, _I64P, _I64P]),
    'ps_pathway_reset': (C.c_int, [_VP]),
    'ps_pathway_fetch_counts': (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_pathway_fetch_members': (C.c_int, [_VP, C.c_int, C.c_int] + [C.POINTER(C.c_uint32)] * 5),
    'ps_pathway_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_pathway_destroy': (None, [_VP]),
    'ps_overlap_create': (C.c_int, [C.c_int, C.c_int, _VP, C.POINTER(_VP)]),
    'ps_overlap_pairs': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_uint32)]),
    'ps_overlap_subset': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_uint32)]),
    'ps_overlap_info': (C.c_int, [_VP, _I64P, _I64P, _I32P]),
    'ps_overlap_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P, _F64P, _I64P]),
    'ps_overlap_destroy': (None, [_VP]),
    'ps_wexcur_create': (C.c_int, [C.c_int, C.c_int, _VP, C.POINTER(_VP)]),
    'ps_wexcur_plane': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int64, _F64P]),
    'ps_wexcur_fetch_counts': (C.c_int, [_VP, _F64P]),
    'ps_wexcur_fetch_bounds': (C.c_int, [_VP, _F64P, _F64P]),
    'ps_wexcur_map': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_wexcur_info': (C.c_int, [_VP, _I64P, _I64P, _F64P]),
    'ps_wexcur_member_weights': (C.c_int, [_VP, C.c_int64, C.POINTER(C.c_uint32)]),
    'ps_wexcur_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_wexcur_destroy': (None, [_VP]),
    'ps_wcontrast_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F64P, C.POINTER(_VP)]),
    'ps_wcontrast_add_sites': (C.c_int, [_VP, _VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_wcontrast_add_project': (C.c_int, [_VP, _VP, _VP, C.c_int, _F64P, _F64P]),
    'ps_wcontrast_merge': (C.c_int, [_VP, _VP, _F64P, _F64P]),
    'ps_wcontrast_info': (C.c_int, [_VP, _F64P, _I64P, _I64P]),
    'ps_wcontrast_fetch': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P]),
    'ps_wcontrast_reset': (C.c_int, [_VP]),
    'ps_wcontrast_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_wcontrast_destroy': (None, [_VP]),
    'ps_modes_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    'ps_modes_reserve': (C.c_int, [_VP, C.c_int64]),
    'ps_modes_set_window': (C.c_int, [_VP, C.c_int]),
    'ps_modes_add': (C.c_int, [_VP, _VP, C.c_int, _I32P, _I32P, _F64P, _F64P, _I32P, C.c_double, C.c_uint32]),
    'ps_modes_add_project': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_modes_add_sites': (C.c_int, [_VP, _VP, C.c_uint32]),
    'ps_modes_add_host': (C.c_int, [_VP, _F64P, C.c_uint32]),
    'ps_modes_merge': (C.c_int, [_VP, _VP]),
    'ps_modes_info': (C.c_int, [_VP, _F64P, _I64P, _I64P, _I64P]),
    'ps_modes_weights': (C.c_int, [_VP, C.c_int64, C.POINTER(C.c_uint32)]),
    'ps_modes_reset': (C.c_int, [_VP]),
    'ps_modes_mean': (C.c_int, [_VP, C.c_int, _F64P]),
    'ps_modes_table': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int64, _F64P]),
    'ps_modes_combine': (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _F64P, _F64P]),
    'ps_modes_fetch_member': (C.c_int, [_VP, C.c_int64, C.c_int, _F64P]),
    'ps_modes_prof': (C.c_int, [_VP, C.c_int, _F64P, _I64P]),
    'ps_modes_destroy': (None, [_VP]),
}

_lib = None


def load():
    """Load the shared library (no HIP call is made).  ImportError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'libparasitoid_hip.so not found at %s; build it with '
            '`python -c "import __graft_entry__ as g; g.build()"` or '
            '`make -C parasitoids_amd/csrc`' % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise ImportError('cannot load %s: %s' % (LIB_PATH, e))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != PS_OK:
        msg = load().ps_last_error()
        raise HipError(rc, msg.decode() if msg else '')


def require_device():
    """ImportError if no usable GPU (mirrors the reference: `import cuda_lib`
    failing makes CalcSol fall back, CalcSol.py:161-172)."""
    lib = load()
    n = lib.ps_device_count()
    if n <= 0:
        msg = lib.ps_last_error()
        raise ImportError('no MI355X/HIP device available: %s' % (msg.decode() if msg else ''))
    return n


def default_device():
    """LOCAL_RANK-aware default device (one process per GPU)."""
    return int(os.environ.get('PARASITOID_DEVICE', os.environ.get('LOCAL_RANK', '0')))


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def p_i32(a):
    return a.ctypes.data_as(_I32P)


def p_i64(a):
    return a.ctypes.data_as(_I64P)


def p_f64(a):
    return a.ctypes.data_as(_F64P)
