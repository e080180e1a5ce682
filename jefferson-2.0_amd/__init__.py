"""jefferson-2.0_amd -- ctypes binding of libjefferson_hip.so (include/jefferson.h).

Plumbing for tests and bench.py; the product is the C ABI.  The directory name is
not an importable identifier, so load it with `jf_load.py` at the repo root
(`from jf_load import jf`).  There is no fallback: if the HIP library is missing
or no GPU is usable, the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# JF_LIB selects an A/B build of the same library (csrc/Makefile `variant`); default = the product
LIB_PATH = os.environ.get("JF_LIB") or os.path.join(_HERE, "libjefferson_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "jefferson.h")
DEBUG_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "jefferson_debug.h")  # taps, timing hooks, tuning switches

JF_OK, JF_ERR_ARG, JF_ERR_RANGE, JF_ERR_DEVICE, JF_ERR_IO, JF_ERR_STATE, JF_ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6
JF_FLAG_CORRECTED_INTERPOLATION = 1
JF_FLAG_NO_INTERP_TABLE = 2
INTERP_ROWS = 131 * 360
JF_MODE_FD_COMPLEX, JF_MODE_FD_BASIC = 0, 1
NUM_HRTF = 710
PAD_LEN = 1024
NC = 513

_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int)


class JfConfig(C.Structure):
    _fields_ = [("frames_per_buffer", C.c_int), ("hrtf_len", C.c_int), ("n_sources", C.c_int),
                ("device", C.c_int), ("max_batch_blocks", C.c_int), ("flags", C.c_uint)]


class JfHrtfGrid(C.Structure):
    _fields_ = [("n_rings", C.c_int), ("ring_elevation", C.POINTER(C.c_float)), ("ring_count", C.POINTER(C.c_int)),
                ("ring_step", C.POINTER(C.c_float))]


JF_MAX_RINGS = 40
JF_MAX_BUSES = 1024
JF_ROOM_MAX_TAPS = 262144
JF_MAX_HRTF_SETS = 64
JF_VOICE_ALWAYS = 255


class JfGridLayout(C.Structure):
    _fields_ = [("n_rings", C.c_int), ("ring_elevation", C.c_float * JF_MAX_RINGS), ("ring_count", C.c_int * JF_MAX_RINGS),
                ("ring_step", C.c_float * JF_MAX_RINGS)]


class JfSofaSet(C.Structure):
    _fields_ = [("n_measurements", C.c_int), ("n_receivers", C.c_int), ("n_samples", C.c_int), ("sample_rate", C.c_double),
                ("ir", C.POINTER(C.c_float)), ("azimuth", C.POINTER(C.c_float)), ("elevation", C.POINTER(C.c_float)),
                ("distance", C.POINTER(C.c_float)), ("delay", C.POINTER(C.c_float)), ("conventions", C.c_char * 48)]


class JfCloudOpaque(C.Structure):
    """jf_cloud: an opaque handle of its own type, so that it cannot be mistaken for an engine's"""
    _fields_ = []


_cloud = C.POINTER(JfCloudOpaque)


class JfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"jefferson error {code}: {msg}")
        self.code = code


_lib = None

_SIGS = {
    "jf_engine_create": (C.c_int, [C.POINTER(JfConfig), _f, C.c_int, C.POINTER(C.c_void_p)]),
    "jf_engine_create_from_dir": (C.c_int, [C.POINTER(JfConfig), C.c_char_p, C.POINTER(C.c_void_p)]),
    "jf_engine_create_grid": (C.c_int, [C.POINTER(JfConfig), C.POINTER(JfHrtfGrid), _f, C.c_int, C.POINTER(C.c_void_p)]),
    "jf_engine_create_sofa": (C.c_int, [C.POINTER(JfConfig), C.c_char_p, C.c_float, C.POINTER(C.c_void_p)]),
    "jf_sofa_read": (C.c_int, [C.c_char_p, C.POINTER(JfSofaSet)]),
    "jf_sofa_release": (None, [C.POINTER(JfSofaSet)]),
    "jf_sofa_taps": (C.c_int, [C.POINTER(JfSofaSet)]),
    "jf_sofa_table": (C.c_int, [C.POINTER(JfSofaSet), C.c_float, C.c_void_p, _f, C.c_int]),
    "jf_debug_hdf5_read": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(C.c_double)), _i, C.POINTER(C.c_ulonglong)]),
    "jf_debug_hdf5_attr": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "jf_cloud_create": (C.c_int, [C.c_size_t, _f, _f, C.c_float, C.POINTER(_cloud)]),
    "jf_cloud_destroy": (None, [_cloud]),
    "jf_cloud_rows": (C.c_int, [_cloud]),
    "jf_cloud_triangles": (C.c_int, [_cloud, _i]),
    "jf_cloud_interpolation": (C.c_int, [_cloud, C.c_float, C.c_float, _i, _f]),
    "jf_cloud_pick": (C.c_int, [_cloud, C.c_float, C.c_float]),
    "jf_engine_create_cloud": (C.c_int, [C.POINTER(JfConfig), _cloud, _f, C.c_int, C.POINTER(C.c_void_p)]),
    "jf_sofa_cloud": (C.c_int, [C.POINTER(JfSofaSet), C.c_float, C.POINTER(_cloud), _f, C.c_int]),
    "jf_engine_create_sofa_cloud": (C.c_int, [C.POINTER(JfConfig), C.c_char_p, C.c_float, C.POINTER(C.c_void_p)]),
    "jf_debug_cloud_walk": (C.c_int, [_cloud, C.c_float, C.c_float]),
    "jf_kemar_grid": (C.c_int, [C.POINTER(JfHrtfGrid)]),
    "jf_grid_rows": (C.c_int, [C.POINTER(JfHrtfGrid)]),
    "jf_grid_from_positions": (C.c_int, [C.c_size_t, _f, _f, C.c_float, C.c_void_p, _i]),
    "jf_grid_interpolation": (C.c_int, [C.POINTER(JfHrtfGrid), C.c_float, C.c_float, _i, _f]),
    "jf_grid_pick": (C.c_int, [C.POINTER(JfHrtfGrid), C.c_float, C.c_float]),
    "jf_table_rows": (C.c_int, [C.c_void_p]),
    "jf_engine_destroy": (None, [C.c_void_p]),
    "jf_last_error": (C.c_char_p, [C.c_void_p]),
    "jf_frames_per_buffer": (C.c_int, [C.c_void_p]),
    "jf_pad_len": (C.c_int, [C.c_void_p]),
    "jf_num_sources": (C.c_int, [C.c_void_p]),
    "jf_source_set_signal": (C.c_int, [C.c_void_p, C.c_int, _f, C.c_size_t]),
    "jf_source_set_live": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_num_live_sources": (C.c_int, [C.c_void_p]),
    "jf_source_set_stream": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "jf_stream_min_capacity": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_source_push": (C.c_int, [C.c_void_p, C.c_int, _f, C.c_int]),
    "jf_source_stream_need": (C.c_longlong, [C.c_void_p, C.c_int, C.c_int]),
    "jf_source_stream_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]),
    "jf_source_stream_rate": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_stream_ratio": (C.c_int, [C.c_int, _i, _i]),
    "jf_stream_table": (C.c_int, [C.c_int, _f]),
    "jf_stream_frames_needed": (C.c_longlong, [C.c_int, C.c_longlong, C.c_longlong]),
    "jf_stream_resample": (C.c_int, [C.c_int, _f, C.c_longlong, C.c_longlong, C.c_longlong, _f]),
    "jf_stream_resample_from": (C.c_int, [C.c_int, _f, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _f]),
    "jf_debug_stream_seek": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong]),
    "jf_debug_input_buffer": (C.c_int, [C.c_void_p, C.c_int, _f, C.c_int]),
    "jf_debug_stream_bytes": (C.c_longlong, [C.c_void_p]),
    "jf_bus_set_output": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "jf_output_min_capacity": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_bus_pull": (C.c_longlong, [C.c_void_p, C.c_int, _f, C.c_longlong]),
    "jf_bus_output_ready": (C.c_longlong, [C.c_void_p, C.c_int]),
    "jf_bus_output_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]),
    "jf_bus_output_rate": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_output_ratio": (C.c_int, [C.c_int, _i, _i, _i]),
    "jf_output_table": (C.c_int, [C.c_int, _f]),
    "jf_output_frames": (C.c_longlong, [C.c_int, C.c_longlong, C.c_longlong]),
    "jf_output_resample": (C.c_int, [C.c_int, _f, C.c_longlong, C.c_longlong, C.c_longlong, _f]),
    "jf_output_resample_from": (C.c_int, [C.c_int, _f, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _f]),
    "jf_debug_output_feed": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_debug_output_seek": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong]),
    "jf_debug_output_bytes": (C.c_longlong, [C.c_void_p]),
    "jf_engine_set_buses": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_num_buses": (C.c_int, [C.c_void_p]),
    "jf_source_set_bus": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_source_bus": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_bus_plan": (C.c_int, [C.c_int, _i, C.c_int, _i, C.c_int, C.c_longlong, C.c_int, _i, _i, _i]),
    "jf_source_share_input": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_source_input_of": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_share_plan": (C.c_int, [C.c_int, _i, _i, _i, _i]),
    "jf_room_set_ir": (C.c_int, [C.c_void_p, _f, _f, C.c_size_t, C.c_float]),
    "jf_room_taps": (C.c_int, [C.c_void_p]),
    "jf_source_set_send": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "jf_source_send": (C.c_float, [C.c_void_p, C.c_int]),
    "jf_debug_room_wet": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_source_set_gain": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int]),
    "jf_source_gain": (C.c_float, [C.c_void_p, C.c_int]),
    "jf_source_set_mute": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "jf_source_muted": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_sources_set_gains": (C.c_int, [C.c_void_p, _f, C.c_int]),
    "jf_batch_set_gains": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_debug_gain_record": (C.c_int, [_i, _f, _i, _f, _i, _i, _i, C.c_float, C.c_float, C.c_int]),
    "jf_profile_read_gain": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_bus_set_master": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int]),
    "jf_bus_master": (C.c_float, [C.c_void_p, C.c_int]),
    "jf_bus_set_limiter": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "jf_bus_limiter": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_engine_set_meters": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_bus_meters": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_debug_master_block": (C.c_int, [_f, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _f, _f, _f]),
    "jf_profile_read_master": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_bus_set_lookahead": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_bus_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_bus_latency": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_master_look_block": (C.c_int, [_f, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _f, _f, _f, _f, _f]),
    "jf_source_set_gate": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int]),
    "jf_source_gate": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _i]),
    "jf_sources_set_gate": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int]),
    "jf_engine_set_input_meters": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_source_levels": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_debug_gate_scan": (C.c_int, [_f, C.c_int, C.c_float, C.c_float, C.c_int, _i, _i]),
    "jf_profile_read_gate": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_bus_set_voices": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int]),
    "jf_bus_voices": (C.c_int, [C.c_void_p, C.c_int, _i, _f]),
    "jf_source_set_priority": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_source_priority": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_source_heard": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_debug_voice_select": (C.c_int, [_f, _i, _i, _i, _i, _f, _i, C.c_int, C.c_int, C.c_int, _f, _f, _f, _i, _f, _i]),
    "jf_profile_read_voices": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_source_set_leveller": (C.c_int, [C.c_void_p, C.c_int, _f]),        # (jf_leveller is six floats)
    "jf_sources_set_leveller": (C.c_int, [C.c_void_p, _f]),
    "jf_source_leveller": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_source_level_gains": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_debug_level_scan": (C.c_int, [_f, C.c_int, _f, _f, _f]),
    "jf_profile_read_level": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_bus_set_range": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "jf_bus_range": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_source_set_range_exempt": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_source_range_exempt": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_source_range_gains": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_range_gain": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _f]),
    "jf_debug_range_scan": (C.c_int, [_f, C.c_int, C.c_int, _f, _f, _f]),
    "jf_profile_read_range": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_debug_range_bytes": (C.c_longlong, [C.c_void_p]),
    "jf_object_set_pose": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_object_get_pose": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_listener_follow_object": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_listener_object": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_object_set_cone": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]),
    "jf_object_cone": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _f]),
    "jf_source_cone_gains": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_cone_gain": (C.c_int, [C.c_float, C.c_float, C.c_float, _f, _f, _f]),
    "jf_process_batch_poses": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _f, _f]),
    "jf_batch_upload_object_poses": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_debug_cone_scan": (C.c_int, [_f, _f, C.c_int, C.c_int, C.c_int, C.c_int, _f, _i, _i, _i, _f, _f]),
    "jf_debug_cone_bytes": (C.c_longlong, [C.c_void_p]),
    "jf_profile_read_cone": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_engine_add_hrtf_set": (C.c_int, [C.c_void_p, _f, C.c_int]),
    "jf_engine_add_hrtf_sofa": (C.c_int, [C.c_void_p, C.c_char_p, C.c_float]),
    "jf_num_hrtf_sets": (C.c_int, [C.c_void_p]),
    "jf_source_set_hrtf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "jf_source_hrtf": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_bus_set_hrtf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "jf_debug_read_hrtf_set": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_debug_set_record": (C.c_int, [_i, _f, _i, _f, _i, _i, _i, C.c_int, C.c_int, C.c_int]),
    "jf_debug_last_set_stage": (C.c_int, [C.c_void_p]),
    "jf_profile_read_sets": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_listener_set_pose": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_listener_get_pose": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_source_set_world": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]),
    "jf_source_get_world": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_position_from_world": (C.c_int, [_f, C.c_float, C.c_float, C.c_float, _f]),
    "jf_process_batch_world": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _f, _f]),
    "jf_batch_upload_world": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_debug_pose_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i, _f, _f, _f]),
    "jf_debug_pose_device_bytes": (C.c_longlong, [C.c_void_p]),
    "jf_profile_read_pose": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "jf_engine_set_objects": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_num_objects": (C.c_int, [C.c_void_p]),
    "jf_source_set_object": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_source_object": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_object_set_world": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]),
    "jf_object_get_world": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_process_batch_objects": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _f, _f]),
    "jf_batch_upload_objects": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_debug_pose_objects_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _i, _i, _f, _f, _f]),
    "jf_submit_block_in": (C.c_int, [C.c_void_p, _f]),
    "jf_process_block_in": (C.c_int, [C.c_void_p, _f, _f]),
    "jf_callback_in": (C.c_int, [C.c_void_p, _f, _f]),
    "jf_process_batch_in": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _f]),
    "jf_source_set_cartesian": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]),
    "jf_source_set_spherical": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]),
    "jf_source_get_position": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_source_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_position_from_spherical": (C.c_int, [C.c_float, C.c_float, C.c_float, _f]),
    "jf_position_from_cartesian": (C.c_int, [C.c_float, C.c_float, C.c_float, _f]),
    "jf_positions_from_spherical": (C.c_int, [C.c_size_t, _f, _f, _f, _f]),
    "jf_interpolation": (C.c_int, [C.c_float, C.c_float, _i, _f]),
    "jf_interpolation_ex": (C.c_int, [C.c_float, C.c_float, C.c_uint, _i, _f]),
    "jf_pick_hrtf": (C.c_int, [C.c_float, C.c_float]),
    "jf_process_block": (C.c_int, [C.c_void_p, _f]),
    "jf_submit_block": (C.c_int, [C.c_void_p]),
    "jf_collect_block": (C.c_int, [C.c_void_p, _f]),
    "jf_callback": (C.c_int, [C.c_void_p, _f]),
    "jf_pa_callback": (C.c_int, [C.c_void_p, C.c_void_p, C.c_ulong, C.c_void_p, C.c_ulong, C.c_void_p]),
    "jf_set_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_set_pause": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_process_batch": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_batch_upload_positions": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_batch_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "jf_synchronize": (C.c_int, [C.c_void_p]),
    "jf_batch_fetch": (C.c_int, [C.c_void_p, C.c_int, _f]),
    "jf_batch_mix_device": (C.c_void_p, [C.c_void_p]),
    "jf_batch_partial_device": (C.c_void_p, [C.c_void_p]),
    "jf_engine_stream": (C.c_void_p, [C.c_void_p]),
    "jf_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "jf_reverb_set_ir": (C.c_int, [C.c_void_p, _f, C.c_size_t, C.c_float]),
    "jf_reverb_rms_gain": (C.c_float, [_f, C.c_size_t, _f, C.c_size_t]),
    "jf_profile_read_reverb": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_profile_read_spectrum": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "jf_profile_set_stride": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_set_source_group": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_read_stamps": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]),
    "jf_debug_source_order": (C.c_int, [C.c_void_p, _i]),
    "jf_debug_set_reverb_form": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_last_block_peak": (C.c_float, [C.c_void_p]),
    "jf_debug_last_kernels": (C.c_char_p, [C.c_void_p]),
    "jf_debug_last_source_group": (C.c_int, [C.c_void_p]),
    "jf_debug_set_grid_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_set_prep_ahead": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_stage_taps": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _f, _f]),
    "jf_debug_copy_from_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "jf_debug_set_rt_max_sources": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_read_table": (C.c_int, [C.c_void_p, _f]),
    "jf_debug_set_interp_table": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_interp_table": (C.c_int, [C.c_void_p]),
    "jf_debug_interp_table_built": (C.c_int, [C.c_void_p]),
    "jf_debug_set_reverb_partitioning": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_set_reverb_async": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_set_reverb_head_fused": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_set_reverb_lazy_state": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_set_reverb_ahead": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_debug_reverb_ahead_pending": (C.c_int, [C.c_void_p]),
    "jf_debug_set_reverb_side_workgroups": (C.c_int, [C.c_void_p, C.c_int]),
    "jf_sources_set_latched": (C.c_int, [C.c_void_p, _f]),
    "jf_device_numa_node": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "jf_pin_thread_to_device": (C.c_int, [C.c_int]),
    "jf_debug_reverb_partitions": (C.c_int, [C.c_void_p, _i, _i, _i]),
    "jf_debug_reverb_schedule": (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_longlong)]),
    "jf_debug_last_run_used_rows": (C.c_int, [C.c_void_p]),
    "jf_debug_count_desc_flags": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "jf_debug_read_table_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _f]),
    "jf_debug_interp_device": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _i, _f, _i]),
    "jf_debug_rfft_device": (C.c_int, [C.c_void_p, C.c_int, _f, _f]),
    "jf_wav_read_mono": (C.c_int, [C.c_char_p, C.POINTER(_f), C.POINTER(C.c_size_t), _i]),
    "jf_wav_write_stereo24": (C.c_int, [C.c_char_p, _f, C.c_size_t, C.c_int]),
    "jf_free": (None, [C.c_void_p]),
}


def exported_symbols():
    """Names every entry point of include/jefferson.h and include/jefferson_debug.h must be exported under."""
    return sorted(_SIGS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JfError(JF_ERR_DEVICE, f"{LIB_PATH} is not built (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _fp(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_f)


def _ip(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_i)


def device_numa_node(device=0):
    """NUMA node of HIP device `device` (-1: the system does not say)."""
    n = C.c_int(-1)
    rc = lib().jf_device_numa_node(int(device), C.byref(n))
    if rc:
        raise JfError(rc, (lib().jf_last_error(None) or b"").decode())
    return n.value


def pin_thread_to_device(device=0):
    """Restrict the calling thread to the CPUs of the device's NUMA node (include/jefferson.h); False if that is not possible."""
    return lib().jf_pin_thread_to_device(int(device)) == 0


def stream_ratio(rate):
    """(L, M) of a stream source's rate: L = 44100 / gcd, M = rate / gcd (jf_stream_ratio); JfError for a rate it refuses"""
    L, M = C.c_int(0), C.c_int(0)
    rc = lib().jf_stream_ratio(int(rate), C.byref(L), C.byref(M))
    if rc:
        raise JfError(rc, "stream_ratio")
    return L.value, M.value


def stream_table(rate):
    """the rate's polyphase table, float32 [L][64] (jf_stream_table)"""
    L, _ = stream_ratio(rate)
    out = np.zeros((L, 64), np.float32)
    rc = lib().jf_stream_table(int(rate), _fp(out))
    if rc:
        raise JfError(rc, "stream_table")
    return out


def stream_frames_needed(rate, t0, n_out):
    """input frames a call of n_out outputs from output position t0 consumes (jf_stream_frames_needed)"""
    n = lib().jf_stream_frames_needed(int(rate), int(t0), int(n_out))
    if n < 0:
        raise JfError(int(n), "stream_frames_needed")
    return int(n)


def stream_resample(rate, x, t0, n_out, x0=0):
    """outputs t0 .. t0 + n_out - 1 of the stream rule on x (jf_stream_resample: the host twin of stream_resample_kernel); x is
    the whole input since t = 0, or with x0 the frames from x0 on (jf_stream_resample_from); every other frame counts as 0"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros(int(n_out), np.float32)
    xp = _fp(x) if x.size else None
    if x0:
        rc = lib().jf_stream_resample_from(int(rate), xp, int(x0), x.size, int(t0), int(n_out), _fp(y))
    else:
        rc = lib().jf_stream_resample(int(rate), xp, x.size, int(t0), int(n_out), _fp(y))
    if rc:
        raise JfError(rc, "stream_resample")
    return y


def output_ratio(rate):
    """(L, M, T) of a bus output's rate: L = rate / gcd phases, M = 44100 / gcd, T taps (jf_output_ratio); JfError for a rate it
    refuses"""
    L, M, T = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib().jf_output_ratio(int(rate), C.byref(L), C.byref(M), C.byref(T))
    if rc:
        raise JfError(rc, "output_ratio")
    return L.value, M.value, T.value


def output_table(rate):
    """the rate's polyphase table, float32 [L][T] (jf_output_table)"""
    L, _, T = output_ratio(rate)
    out = np.zeros((L, T), np.float32)
    rc = lib().jf_output_table(int(rate), _fp(out))
    if rc:
        raise JfError(rc, "output_table")
    return out


def output_frames(rate, n0, n):
    """output frames a call that renders n frames after n0 yields: produced(n0 + n) - produced(n0) (jf_output_frames)"""
    r = lib().jf_output_frames(int(rate), int(n0), int(n))
    if r < 0:
        raise JfError(int(r), "output_frames")
    return int(r)


def output_resample(rate, x, u0, n_out, x0=0):
    """output frames u0 .. u0 + n_out - 1, [n_out][2], of the bus output rule on the stereo frames x[n][2] (jf_output_resample:
    the host twin of output_resample_kernel); x is the whole input since frame 0, or with x0 the frames from x0 on
    (jf_output_resample_from); every other frame counts as 0"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 2)
    y = np.zeros((int(n_out), 2), np.float32)
    xp = _fp(x) if x.size else None
    yp = _fp(y) if y.size else None
    if x0:
        rc = lib().jf_output_resample_from(int(rate), xp, int(x0), x.shape[0], int(u0), int(n_out), yp)
    else:
        rc = lib().jf_output_resample(int(rate), xp, x.shape[0], int(u0), int(n_out), yp)
    if rc:
        raise JfError(rc, "output_resample")
    return y


def position_from_spherical(ele, azi, r):
    o = np.zeros(5, np.float32)
    rc = lib().jf_position_from_spherical(ele, azi, r, _fp(o))
    if rc:
        raise JfError(rc, "position_from_spherical")
    return o


def positions_from_spherical(ele, azi, r):
    """Vectorised: arrays of equal shape -> float32 [..., 5] latched records."""
    ele = np.ascontiguousarray(ele, np.float32)
    azi = np.ascontiguousarray(np.broadcast_to(azi, ele.shape), np.float32)
    r = np.ascontiguousarray(np.broadcast_to(r, ele.shape), np.float32)
    out = np.zeros(ele.shape + (5,), np.float32)
    rc = lib().jf_positions_from_spherical(ele.size, _fp(ele), _fp(azi), _fp(r), _fp(out))
    if rc:
        raise JfError(rc, "positions_from_spherical")
    return out


def position_from_cartesian(x, y, z):
    o = np.zeros(5, np.float32)
    rc = lib().jf_position_from_cartesian(x, y, z, _fp(o))
    return None if rc else o


def position_from_world(pose, x, y, z):
    """the latched record of a source at world (x, y, z) for a listener at pose {cx, cy, cz, qw, qx, qy, qz}
    (include/jefferson.h: jf_position_from_world -- the host twin of pose_kernel); JfError for arguments it refuses"""
    pose = np.ascontiguousarray(pose, np.float32)
    assert pose.shape == (7,)
    o = np.zeros(5, np.float32)
    rc = lib().jf_position_from_world(_fp(pose), x, y, z, _fp(o))
    if rc:
        raise JfError(rc, "position_from_world")
    return o


def positions_from_world(poses, world):
    """position_from_world over arrays: poses [..., 7] and world [..., 3] of equal leading shape -> [..., 5]"""
    poses = np.ascontiguousarray(poses, np.float32)
    world = np.ascontiguousarray(world, np.float32)
    assert poses.shape[:-1] == world.shape[:-1] and poses.shape[-1] == 7 and world.shape[-1] == 3
    out = np.zeros(world.shape[:-1] + (5,), np.float32)
    q, w, o = poses.reshape(-1, 7), world.reshape(-1, 3), out.reshape(-1, 5)
    fn = lib().jf_position_from_world
    base_q, base_o = q.ctypes.data, o.ctypes.data
    for i in range(len(w)):
        rc = fn(C.cast(base_q + 28 * i, _f), w[i, 0], w[i, 1], w[i, 2], C.cast(base_o + 20 * i, _f))
        if rc:
            raise JfError(rc, f"position_from_world, record {i}")
    return out


def interpolation(ele, azi, flags=0):
    idx = np.zeros(4, np.int32)
    om = np.zeros(6, np.float32)
    rc = lib().jf_interpolation_ex(ele, azi, flags, _ip(idx), _fp(om)) if flags else \
        lib().jf_interpolation(ele, azi, _ip(idx), _fp(om))
    return None if rc else (idx, om)


def gain_record(rows_new, w_new, rows_old, w_old, n_new, n_old, flags, g0, g1, canon):
    """jf_debug_gain_record (host logic only): the per-source gain rule on one descriptor ->
    (changed, rows_new, w_new, rows_old, w_old, n_new, n_old, flags)"""
    rn, ro = np.array(rows_new, np.int32), np.array(rows_old, np.int32)
    wn, wo = np.array(w_new, np.float32), np.array(w_old, np.float32)
    assert rn.shape == ro.shape == wn.shape == wo.shape == (4,)
    c = np.array([n_new, n_old, flags], np.int32)
    rc = lib().jf_debug_gain_record(_ip(rn), _fp(wn), _ip(ro), _fp(wo), _ip(c[0:1]), _ip(c[1:2]), _ip(c[2:3]),
                                    float(g0), float(g1), int(canon))
    if rc < 0:
        raise JfError(rc, "gain_record")
    return bool(rc), rn, wn, ro, wo, int(c[0]), int(c[1]), int(c[2])


def set_record(rows_new, w_new, rows_old, w_old, n_new, n_old, flags, off0, off1, canon):
    """jf_debug_set_record (host logic only): the HRTF-set rule on one descriptor ->
    (changed, rows_new, w_new, rows_old, w_old, n_new, n_old, flags)"""
    rn = np.ascontiguousarray(rows_new, np.int32).copy()
    wn = np.ascontiguousarray(w_new, np.float32).copy()
    ro = np.ascontiguousarray(rows_old, np.int32).copy()
    wo = np.ascontiguousarray(w_old, np.float32).copy()
    c = np.array([n_new, n_old, flags], np.int32)
    rc = lib().jf_debug_set_record(_ip(rn), _fp(wn), _ip(ro), _fp(wo), _ip(c[0:1]), _ip(c[1:2]), _ip(c[2:3]),
                                   int(off0), int(off1), int(canon))
    if rc < 0:
        raise JfError(rc, "set_record")
    return bool(rc), rn, wn, ro, wo, int(c[0]), int(c[1]), int(c[2])


def reverb_schedule(j0, K, M, fut_m):
    """jf_debug_reverb_schedule as a dict (host logic only)"""
    out = (C.c_longlong * 16)()
    rc = lib().jf_debug_reverb_schedule(j0, K, M, fut_m, out)
    if rc:
        raise JfError(rc, "reverb_schedule")
    names = ("m_lo", "n_tr", "ma", "n_mid", "n_ranges", "kb0", "kn0", "kb1", "kn1", "copy_lo", "copy_hi", "skip_lo", "skip_hi",
             "tail_early", "tail_late", "fut_m")
    return {n: int(v) for n, v in zip(names, out)}


def bus_plan(bus, n_buses, row_key=None, pinned=0, n_items=0, pad_len=1024):
    """jf_debug_bus_plan (host logic only): (G, order[S], list[S / G], seg[n_buses + 1])"""
    bus = np.ascontiguousarray(bus, np.int32)
    S = len(bus)
    key = None if row_key is None else np.ascontiguousarray(row_key, np.int32)
    order, lst, seg = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(n_buses + 1, np.int32)
    G = lib().jf_debug_bus_plan(S, _ip(bus), int(n_buses), None if key is None else _ip(key), int(pinned), int(n_items),
                                int(pad_len), _ip(order), _ip(lst), _ip(seg))
    if G <= 0:
        raise JfError(G, "bus_plan")
    return G, order, lst[:S // G], seg


def share_plan(root):
    """jf_debug_share_plan (host logic only): (n_slots, xslot[S], seg[n_slots + 1], list[seg[-1]])"""
    root = np.ascontiguousarray(root, np.int32)
    S = len(root)
    xslot, seg, lst = np.zeros(S, np.int32), np.zeros(S // 2 + 2, np.int32), np.zeros(S, np.int32)
    n = lib().jf_debug_share_plan(S, _ip(root), _ip(xslot), _ip(seg), _ip(lst))
    if n < 0:
        raise JfError(n, "share_plan")
    return n, xslot, seg[:n + 1], lst[:seg[n]]


def pick_hrtf(ele, azi):
    return lib().jf_pick_hrtf(ele, azi)


def master_block(x, m_prev=1.0, m_new=1.0, ceiling=0.0, release=1.0, g_prev=1.0):
    """jf_debug_master_block (host logic only): the bus-master rule on one block x [B][2] (or [2B]) ->
    (out [2B], meters [4] = {peak_in, peak_out, sumsq_out, gain}, the limiter gain after the block)"""
    x = np.ascontiguousarray(x, np.float32).ravel()
    assert x.size % 2 == 0
    out, m, g = np.zeros_like(x), np.zeros(4, np.float32), np.array([g_prev], np.float32)
    rc = lib().jf_debug_master_block(_fp(x), x.size // 2, m_prev, m_new, ceiling, release, _fp(g), _fp(out), _fp(m))
    if rc:
        raise JfError(rc, "master_block")
    return out, m, g[0]


def master_look_block(x, held, p_held=0.0, m_prev=1.0, m_new=1.0, ceiling=0.0, release=1.0, g_prev=1.0):
    """jf_debug_master_look_block (host logic only): the look-ahead form of the bus-master rule.  x [2B] comes in, held [2B]
    (the block before, master gain applied; zeros at the start) goes out -> (out [2B], meters [4], the new held block [2B], its
    peak, the limiter gain after the block)"""
    x = np.ascontiguousarray(x, np.float32).ravel()
    h = np.array(held, np.float32).ravel()
    assert x.size % 2 == 0 and h.size == x.size
    out, m = np.zeros_like(x), np.zeros(4, np.float32)
    p, g = np.array([p_held], np.float32), np.array([g_prev], np.float32)
    rc = lib().jf_debug_master_look_block(_fp(x), x.size // 2, m_prev, m_new, ceiling, release, _fp(h), _fp(p), _fp(g), _fp(out), _fp(m))
    if rc:
        raise JfError(rc, "master_look_block")
    return out, m, h, p[0], g[0]


def gate_scan(peaks, open, close, hold, state=(0, 0)):
    """jf_debug_gate_scan (host logic only): the voice-gate rule over a sequence of block levels ->
    (gates [n] int32, the state (is_open, hold_left) after the sequence)"""
    peaks = np.ascontiguousarray(peaks, np.float32).ravel()
    st, out = np.array(state, np.int32), np.zeros(max(len(peaks), 1), np.int32)
    rc = lib().jf_debug_gate_scan(_fp(peaks), len(peaks), open, close, int(hold), _ip(st), _ip(out))
    if rc:
        raise JfError(rc, "gate_scan")
    return out[:len(peaks)], (int(st[0]), int(st[1]))


LEVELLER_FIELDS = ("target", "floor", "min_gain", "max_gain", "fall", "rise")


def _leveller(target, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0):
    """jf_leveller as the six float32 the boundary takes"""
    return np.array([target, floor, min_gain, max_gain, fall, rise], np.float32)


def level_scan(peaks, target, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0, a_prev=1.0):
    """jf_debug_level_scan (host logic only): the levelling rule over a sequence of block levels ->
    (a [n] float32, a_prev after the sequence)"""
    peaks = np.ascontiguousarray(peaks, np.float32).ravel()
    st, out = np.array([a_prev], np.float32), np.zeros(max(len(peaks), 1), np.float32)
    rc = lib().jf_debug_level_scan(_fp(peaks), len(peaks), _fp(_leveller(target, floor, min_gain, max_gain, fall, rise)), _fp(st), _fp(out))
    if rc:
        raise JfError(rc, "level_scan")
    return out[:len(peaks)], st[0]


def range_gain(near, far, x, y, z):
    """jf_range_gain (host logic only): how much a listener with the hearing range {near, far} hears of a talker at the
    head-relative (x, y, z) -> float32; JfError for a range the setter would refuse"""
    out = np.zeros(1, np.float32)
    rc = lib().jf_range_gain(float(near), float(far), float(x), float(y), float(z), _fp(out))
    if rc:
        raise JfError(rc, "range_gain")
    return out[0]


def range_scan(pos, near, far, h_prev=None):
    """jf_debug_range_scan (host logic only): the hearing-range rule over one run.  pos [K][S][5] records; near, far [S] per
    source ({0, 0}: exempt or no range); h_prev [S] (ones) -> (h [K][S] float32, h_prev after the run)"""
    pos = np.ascontiguousarray(pos, np.float32)
    K, S = pos.shape[0], pos.shape[1]
    par = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(near, np.float32), (S,)),
                                         np.broadcast_to(np.asarray(far, np.float32), (S,))]), np.float32)
    st = np.ones(S, np.float32) if h_prev is None else np.array(h_prev, np.float32).reshape(S).copy()
    out = np.zeros((max(K, 1), S), np.float32)
    rc = lib().jf_debug_range_scan(_fp(pos), K, S, _fp(par), _fp(st), _fp(out))
    if rc:
        raise JfError(rc, "range_scan")
    return out[:K], st


def cone_gain(inner, outer, outer_gain, talker_pose, listener_centre):
    """jf_cone_gain (host logic only): how much of a talker at talker_pose {x, y, z, qw, qx, qy, qz} with the cone {inner,
    outer, outer_gain} (degrees, degrees, gain) is heard from listener_centre -> float32; JfError for a cone or a pose the
    setters would refuse"""
    tp = np.ascontiguousarray(talker_pose, np.float32).reshape(7)
    c = np.ascontiguousarray(listener_centre, np.float32).reshape(3)
    out = np.zeros(1, np.float32)
    rc = lib().jf_cone_gain(float(inner), float(outer), float(outer_gain), _fp(tp), _fp(c), _fp(out))
    if rc:
        raise JfError(rc, "cone_gain")
    return out[0]


def cone_scan(object_poses, listener_poses, par, object_of, bus, follow, d_prev=None):
    """jf_debug_cone_scan (host logic only): the cone rule over one run.  object_poses [K][n_obj][7], listener_poses
    [K][n_buses][7]; par [3][S] inner, outer, outer_gain per source; object_of, bus, follow [S] (follow: the object the listener
    of the source's bus follows, -1: none); d_prev [S] (ones) -> (d [K][S] float32, d_prev after the run)"""
    op = np.ascontiguousarray(object_poses, np.float32)
    lp = np.ascontiguousarray(listener_poses, np.float32)
    K, no, nb = op.shape[0], op.shape[1], lp.shape[1]
    par = np.ascontiguousarray(par, np.float32)
    S = par.shape[1]
    assert op.shape == (K, no, 7) and lp.shape == (K, nb, 7) and par.shape == (3, S)
    m = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.int32), (S,)), np.int32) for a in (object_of, bus, follow)]
    st = np.ones(S, np.float32) if d_prev is None else np.array(d_prev, np.float32).reshape(S).copy()
    out = np.zeros((max(K, 1), S), np.float32)
    rc = lib().jf_debug_cone_scan(_fp(op), _fp(lp), K, S, no, nb, _fp(par), _ip(m[0]), _ip(m[1]), _ip(m[2]), _fp(st), _fp(out))
    if rc:
        raise JfError(rc, "cone_scan")
    return out[:K], st


def voice_select(peak, root, bus, priority, max_voices, release, g_eff, g_eff_prev, env_prev=None, heard_prev=None, snap=None):
    """jf_debug_voice_select (host logic only): the voice-limit rule over one run.  peak, g_eff [K][S]; root, bus, priority,
    g_eff_prev [S]; max_voices, release, snap [n_buses]; the state env_prev (zeros), heard_prev (ones) [S] ->
    (g_out [K][S], g_out_prev [S], env [K][S], keep [K][S] int32, (env_prev, heard_prev) after the run)"""
    g_out = np.array(g_eff, np.float32, ndmin=2)
    K, S = g_out.shape
    g_out = np.ascontiguousarray(g_out)
    peak = np.ascontiguousarray(np.asarray(peak, np.float32).reshape(K, S))
    g_prev = np.array(g_eff_prev, np.float32).reshape(S).copy()
    ints = lambda a: np.ascontiguousarray(np.asarray(a, np.int32).ravel())
    root, bus, priority, max_voices = ints(root), ints(bus), ints(priority), ints(max_voices)
    release = np.ascontiguousarray(np.asarray(release, np.float32).ravel())
    nb = len(max_voices)
    snap = np.zeros(nb, np.int32) if snap is None else ints(snap)
    env_io = np.zeros(S, np.float32) if env_prev is None else np.array(env_prev, np.float32).reshape(S).copy()
    heard_io = np.ones(S, np.int32) if heard_prev is None else np.array(heard_prev, np.int32).reshape(S).copy()
    if not (len(root) == len(bus) == len(priority) == S and len(release) == len(snap) == nb):
        raise JfError(JF_ERR_ARG, "voice_select: array lengths")
    env, keep = np.zeros((max(K, 1), S), np.float32), np.zeros((max(K, 1), S), np.int32)
    rc = lib().jf_debug_voice_select(_fp(peak), _ip(root), _ip(bus), _ip(priority), _ip(max_voices), _fp(release), _ip(snap), S, K,
                                     nb, _fp(g_out), _fp(g_prev), _fp(env_io), _ip(heard_io), _fp(env), _ip(keep))
    if rc:
        raise JfError(rc, "voice_select")
    return g_out, g_prev, env[:K], keep[:K], (env_io, heard_io)


def reverb_rms_gain(signal, ir):
    signal = np.ascontiguousarray(signal, np.float32)
    ir = np.ascontiguousarray(ir, np.float32)
    return float(lib().jf_reverb_rms_gain(_fp(signal), len(signal), _fp(ir), len(ir)))


def wav_read_mono(path):
    p = _f()
    n = C.c_size_t()
    fs = C.c_int()
    rc = lib().jf_wav_read_mono(path.encode(), C.byref(p), C.byref(n), C.byref(fs))
    if rc:
        raise JfError(rc, lib().jf_last_error(None).decode())
    out = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32)
    lib().jf_free(p)
    return out, fs.value


def wav_write_stereo24(path, interleaved, fs=44100):
    a = np.ascontiguousarray(interleaved, np.float32).reshape(-1)
    rc = lib().jf_wav_write_stereo24(path.encode(), _fp(a), len(a) // 2, fs)
    if rc:
        raise JfError(rc, lib().jf_last_error(None).decode())


class SofaSet:
    """include/jefferson.h: jf_sofa_read -- the variables of a SOFA file as arrays (copies; the library's buffers are released)."""

    def __init__(self, path):
        self.c = None
        c = JfSofaSet()
        rc = lib().jf_sofa_read(os.fsencode(path), C.byref(c))
        if rc:
            raise JfError(rc, lib().jf_last_error(None).decode())
        self.c = c
        M, R, N = c.n_measurements, c.n_receivers, c.n_samples
        self.M, self.R, self.N, self.sample_rate = M, R, N, c.sample_rate
        self.conventions = c.conventions.decode(errors="replace")
        arr = lambda p, shape: np.ctypeslib.as_array(p, shape=shape).copy()
        self.ir = arr(c.ir, (M, R, N))
        self.azimuth, self.elevation, self.distance = arr(c.azimuth, (M,)), arr(c.elevation, (M,)), arr(c.distance, (M,))
        self.delay = arr(c.delay, (M, R))

    def taps(self):
        n = lib().jf_sofa_taps(C.byref(self.c))
        if n < 0:
            raise JfError(n, lib().jf_last_error(None).decode())
        return n

    def table(self, tol_deg=0.05, taps=None):
        """(Grid, hrir [M][2][taps]) for Engine(..., hrir=, grid=): include/jefferson.h: jf_sofa_table"""
        taps = self.taps() if taps is None else taps
        lay = JfGridLayout()
        hrir = np.zeros((self.M, 2, taps), np.float32)
        rc = lib().jf_sofa_table(C.byref(self.c), tol_deg, C.byref(lay), _fp(hrir), taps)
        if rc:
            raise JfError(rc, lib().jf_last_error(None).decode())
        n = lay.n_rings
        return Grid(list(lay.ring_elevation[:n]), list(lay.ring_count[:n]), list(lay.ring_step[:n])), hrir

    def cloud(self, tol_deg=0.05, taps=None):
        """(Cloud, hrir [M][2][taps]) for Engine(..., hrir=, cloud=), rows in file order: include/jefferson.h: jf_sofa_cloud"""
        taps = self.taps() if taps is None else taps
        hrir = np.zeros((self.M, 2, taps), np.float32)
        h = _cloud()
        rc = lib().jf_sofa_cloud(C.byref(self.c), tol_deg, C.byref(h), _fp(hrir), taps)
        if rc:
            raise JfError(rc, lib().jf_last_error(None).decode())
        return Cloud._adopt(h), hrir

    def close(self):
        if self.c is not None:
            lib().jf_sofa_release(C.byref(self.c))
            self.c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hdf5_read(path, dataset):
    """tests: a numeric dataset of an HDF5 file through the library's own reader (jf_hdf5.c), float64"""
    p = C.POINTER(C.c_double)()
    rank = C.c_int()
    dims = (C.c_ulonglong * 8)()
    rc = lib().jf_debug_hdf5_read(os.fsencode(path), dataset.encode(), C.byref(p), C.byref(rank), dims)
    if rc:
        raise JfError(rc, lib().jf_last_error(None).decode())
    shape = tuple(int(dims[i]) for i in range(rank.value))
    n = int(np.prod(shape)) if shape else 1
    out = np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(shape) if n else np.zeros(shape)
    lib().jf_free(p)
    return out


def hdf5_attr(path, obj, attr):
    """tests: a string attribute (None if the object has none of that name)"""
    buf = C.create_string_buffer(512)
    rc = lib().jf_debug_hdf5_attr(os.fsencode(path), obj.encode(), attr.encode(), buf, 512)
    if rc == JF_ERR_ARG:
        return None
    if rc:
        raise JfError(rc, lib().jf_last_error(None).decode())
    return buf.value.decode(errors="replace")


class Grid:
    """include/jefferson.h: jf_hrtf_grid (keeps its arrays alive)."""

    def __init__(self, ring_elevation, ring_count, ring_step=None):
        self.ele = np.ascontiguousarray(ring_elevation, np.float32)
        self.count = np.ascontiguousarray(ring_count, np.int32)
        self.step = None if ring_step is None else np.ascontiguousarray(ring_step, np.float32)
        assert len(self.ele) == len(self.count) and (self.step is None or len(self.step) == len(self.ele))
        self.c = JfHrtfGrid(len(self.ele), _fp(self.ele), _ip(self.count), _fp(self.step) if self.step is not None else None)

    @staticmethod
    def kemar():
        g = JfHrtfGrid()
        assert lib().jf_kemar_grid(C.byref(g)) == 0
        n = g.n_rings
        return Grid([g.ring_elevation[i] for i in range(n)], [g.ring_count[i] for i in range(n)],
                    [g.ring_step[i] for i in range(n)])

    @staticmethod
    def from_positions(azimuth_deg, elevation_deg, tol_deg=0.05):
        """(Grid, row_of): the rings of a set from its measurements' directions (include/jefferson.h: jf_grid_from_positions)"""
        az = np.ascontiguousarray(azimuth_deg, np.float32)
        el = np.ascontiguousarray(elevation_deg, np.float32)
        assert az.shape == el.shape and az.ndim == 1
        lay = JfGridLayout()
        row_of = np.zeros(len(az), np.int32)
        rc = lib().jf_grid_from_positions(len(az), _fp(az), _fp(el), tol_deg, C.byref(lay), _ip(row_of))
        if rc:
            raise JfError(rc, lib().jf_last_error(None).decode())
        n = lay.n_rings
        return Grid(list(lay.ring_elevation[:n]), list(lay.ring_count[:n]), list(lay.ring_step[:n])), row_of

    def rows(self):
        n = lib().jf_grid_rows(C.byref(self.c))
        if n < 0:
            raise JfError(n, lib().jf_last_error(None).decode())
        return n

    def interpolation(self, ele, azi):
        idx = np.zeros(4, np.int32)
        om = np.zeros(6, np.float32)
        rc = lib().jf_grid_interpolation(C.byref(self.c), ele, azi, _ip(idx), _fp(om))
        return None if rc else (idx, om)

    def pick(self, ele, azi):
        return lib().jf_grid_pick(C.byref(self.c), ele, azi)


class Cloud:
    """include/jefferson.h: jf_cloud -- a set on arbitrary directions: direction i is table row i."""

    def __init__(self, azimuth_deg, elevation_deg, tol_deg=0.05):
        self.h = None
        az = np.ascontiguousarray(azimuth_deg, np.float32)
        el = np.ascontiguousarray(elevation_deg, np.float32)
        assert az.shape == el.shape and az.ndim == 1
        h = _cloud()
        rc = lib().jf_cloud_create(len(az), _fp(az), _fp(el), tol_deg, C.byref(h))
        if rc:
            raise JfError(rc, lib().jf_last_error(None).decode())
        self.h = h

    @classmethod
    def _adopt(cls, h):
        c = cls.__new__(cls)
        c.h = h
        return c

    def close(self):
        if getattr(self, "h", None):
            lib().jf_cloud_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self):
        return lib().jf_cloud_rows(self.h)

    def triangles(self):
        """[2n - 4][3] table rows, every triangle outward"""
        n = lib().jf_cloud_triangles(self.h, None)
        tri = np.zeros((n, 3), np.int32)
        assert lib().jf_cloud_triangles(self.h, _ip(tri)) == n
        return tri

    def interpolation(self, ele, azi):
        """(rows[3], w[3]) or None for a position without an answer"""
        rows = np.zeros(3, np.int32)
        w = np.zeros(3, np.float32)
        n = lib().jf_cloud_interpolation(self.h, ele, azi, _ip(rows), _fp(w))
        return (rows, w) if n > 0 else None

    def interpolation_many(self, ele, azi):
        """rows [n][3], w [n][3], terms [n] for arrays of positions"""
        ele = np.ascontiguousarray(ele, np.float32)
        azi = np.ascontiguousarray(azi, np.float32)
        n = len(ele)
        rows = np.zeros((n, 3), np.int32)
        w = np.zeros((n, 3), np.float32)
        nt = np.zeros(n, np.int32)
        fn, h = lib().jf_cloud_interpolation, self.h
        for i in range(n):
            nt[i] = fn(h, ele[i], azi[i], rows[i].ctypes.data_as(_i), w[i].ctypes.data_as(_f))
        return rows, w, nt

    def pick(self, ele, azi):
        return lib().jf_cloud_pick(self.h, ele, azi)

    def walk(self, ele, azi):
        """triangle records the rule's walk reads for this position (include/jefferson_debug.h: jf_debug_cloud_walk)"""
        return lib().jf_debug_cloud_walk(self.h, ele, azi)


class Engine:
    """Thin object wrapper; method names follow the C ABI."""

    def __init__(self, B, hrtf_len, n_sources, hrir=None, hrir_dir=None, device=0, max_batch_blocks=1, flags=0, grid=None,
                 sofa=None, sofa_tol_deg=0.05, cloud=None, sofa_cloud=None):
        L = lib()
        cfg = JfConfig(B, hrtf_len, n_sources, device, max_batch_blocks, flags)
        h = C.c_void_p()
        if sofa_cloud is not None:
            rc = L.jf_engine_create_sofa_cloud(C.byref(cfg), os.fsencode(sofa_cloud), sofa_tol_deg, C.byref(h))
        elif cloud is not None:
            hrir = np.ascontiguousarray(hrir, np.float32)
            assert hrir.ndim == 3 and hrir.shape[0] == cloud.rows() and hrir.shape[1] == 2  # the C side reads rows x 2 x taps floats
            rc = L.jf_engine_create_cloud(C.byref(cfg), cloud.h, _fp(hrir), hrir.shape[2], C.byref(h))
        elif sofa is not None:
            rc = L.jf_engine_create_sofa(C.byref(cfg), os.fsencode(sofa), sofa_tol_deg, C.byref(h))
        elif grid is not None:
            hrir = np.ascontiguousarray(hrir, np.float32)
            assert hrir.ndim == 3 and hrir.shape[0] == grid.rows() and hrir.shape[1] == 2  # the C side reads rows x 2 x taps floats
            self._grid = grid
            rc = L.jf_engine_create_grid(C.byref(cfg), C.byref(grid.c), _fp(hrir), hrir.shape[2], C.byref(h))
        elif hrir_dir is not None:
            rc = L.jf_engine_create_from_dir(C.byref(cfg), hrir_dir.encode(), C.byref(h))
        else:
            hrir = np.ascontiguousarray(hrir, np.float32)
            assert hrir.shape[0] == NUM_HRTF and hrir.shape[1] == 2
            rc = L.jf_engine_create(C.byref(cfg), _fp(hrir), hrir.shape[2], C.byref(h))
        if rc:
            raise JfError(rc, L.jf_last_error(None).decode())
        self.h = h
        self.B, self.S, self.maxK = B, n_sources, max_batch_blocks
        self.N = L.jf_pad_len(h)

    def close(self):
        if getattr(self, "h", None):
            lib().jf_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise JfError(rc, lib().jf_last_error(self.h).decode())

    def set_signal(self, s, mono):
        mono = np.ascontiguousarray(mono, np.float32)
        self._chk(lib().jf_source_set_signal(self.h, s, _fp(mono), len(mono)))

    def set_spherical(self, s, ele, azi, r):
        return lib().jf_source_set_spherical(self.h, s, ele, azi, r)

    def set_cartesian(self, s, x, y, z):
        return lib().jf_source_set_cartesian(self.h, s, x, y, z)

    def get_position(self, s):
        o = np.zeros(6, np.float32)
        self._chk(lib().jf_source_get_position(self.h, s, _fp(o)))
        return o

    def reset(self, s):
        self._chk(lib().jf_source_reset(self.h, s))

    def set_live(self, s, on=True):
        """source s takes its samples from the processing calls' `inp` (include/jefferson.h: jf_source_set_live)"""
        self._chk(lib().jf_source_set_live(self.h, s, int(bool(on))))

    def n_live(self):
        return lib().jf_num_live_sources(self.h)

    def stream_min_capacity(self, rate):
        c = lib().jf_stream_min_capacity(self.h, int(rate))
        if c < 0:
            raise JfError(c, "stream_min_capacity")
        return c

    def set_stream(self, s, rate, capacity=None):
        """source s takes packets at `rate` Hz through push() (include/jefferson.h: jf_source_set_stream); rate 0: resident and
        silent again.  capacity None: the minimum plus a tenth of a second"""
        if capacity is None:
            capacity = 0 if not rate else self.stream_min_capacity(rate) + int(rate) // 10
        self._chk(lib().jf_source_set_stream(self.h, int(s), int(rate), int(capacity)))

    def push(self, s, frames):
        frames = np.ascontiguousarray(frames, np.float32).reshape(-1)
        self._chk(lib().jf_source_push(self.h, int(s), _fp(frames) if frames.size else None, frames.size))

    def stream_need(self, s, n_blocks=1):
        n = lib().jf_source_stream_need(self.h, int(s), int(n_blocks))
        if n < 0:
            raise JfError(int(n), "stream_need")
        return int(n)

    def stream_stats(self, s):
        """{pushed, consumed, zeros_inserted, queued} (jf_source_stream_stats)"""
        o = (C.c_ulonglong * 4)()
        self._chk(lib().jf_source_stream_stats(self.h, int(s), o))
        return dict(zip(("pushed", "consumed", "zeros_inserted", "queued"), (int(v) for v in o)))

    def stream_rate(self, s):
        return lib().jf_source_stream_rate(self.h, int(s))

    def stream_seek(self, s, t_out):
        self._chk(lib().jf_debug_stream_seek(self.h, int(s), int(t_out)))

    def stream_bytes(self):
        return int(lib().jf_debug_stream_bytes(self.h))

    def input_buffer(self, s):
        """the device buffer a live or stream source's samples are put into (jf_debug_input_buffer)"""
        n = lib().jf_debug_input_buffer(self.h, int(s), None, 0)
        if n < 0:
            self._chk(n)
        out = np.zeros(n, np.float32)
        self._chk(min(0, lib().jf_debug_input_buffer(self.h, int(s), _fp(out), n)))
        return out

    def output_min_capacity(self, rate):
        c = lib().jf_output_min_capacity(self.h, int(rate))
        if c < 0:
            raise JfError(c, "output_min_capacity")
        return c

    def set_output(self, bus, rate, capacity=None):
        """bus's mix once more at `rate` Hz, pulled through pull() (include/jefferson.h: jf_bus_set_output); rate 0: no output.
        capacity None: the minimum plus a tenth of a second"""
        if capacity is None:
            capacity = 0 if not rate else self.output_min_capacity(rate) + int(rate) // 10
        self._chk(lib().jf_bus_set_output(self.h, int(bus), int(rate), int(capacity)))

    def pull(self, bus, n):
        """up to n stereo frames of the bus's output, [m][2] with m <= n (jf_bus_pull)"""
        out = np.zeros((max(int(n), 0), 2), np.float32)
        m = lib().jf_bus_pull(self.h, int(bus), _fp(out) if out.size else None, int(n))
        if m < 0:
            self._chk(int(m))
        return out[:m]

    def output_ready(self, bus):
        n = lib().jf_bus_output_ready(self.h, int(bus))
        if n < 0:
            raise JfError(int(n), "output_ready")
        return int(n)

    def output_stats(self, bus):
        """{produced, pulled, dropped, queued} (jf_bus_output_stats)"""
        o = (C.c_ulonglong * 4)()
        self._chk(lib().jf_bus_output_stats(self.h, int(bus), o))
        return dict(zip(("produced", "pulled", "dropped", "queued"), (int(v) for v in o)))

    def output_rate(self, bus):
        return lib().jf_bus_output_rate(self.h, int(bus))

    def output_bytes(self):
        return int(lib().jf_debug_output_bytes(self.h))

    def output_feed(self, x):
        """runs only the output stage on the mix x[n_buses][K][2B] (jf_debug_output_feed)"""
        x = np.ascontiguousarray(x, np.float32).reshape(self.n_buses, -1, 2 * self.B)
        self._chk(lib().jf_debug_output_feed(self.h, x.shape[1], _fp(x)))

    def output_seek(self, bus, n_in):
        self._chk(lib().jf_debug_output_seek(self.h, int(bus), int(n_in)))

    def set_buses(self, n):
        """n stereo mixes (include/jefferson.h: jf_engine_set_buses); with more than one, every array a processing call
        returns gains a leading bus axis"""
        self._chk(lib().jf_engine_set_buses(self.h, int(n)))

    def set_bus(self, s, b):
        self._chk(lib().jf_source_set_bus(self.h, int(s), int(b)))

    @property
    def n_buses(self):
        return lib().jf_num_buses(self.h)

    def bus(self, s):
        b = lib().jf_source_bus(self.h, int(s))
        if b < 0:
            raise JfError(b, "bad source index")
        return b

    def share_input(self, s, of):
        """source s plays the input of source `of` (include/jefferson.h: jf_source_share_input); of < 0 or of == s detaches"""
        self._chk(lib().jf_source_share_input(self.h, int(s), int(of)))

    def input_of(self, s):
        r = lib().jf_source_input_of(self.h, int(s))
        if r < 0:
            raise JfError(r, "bad source index")
        return r

    def set_room(self, ir_left, ir_right=None, gain=1.0):
        """one stereo room per output bus (include/jefferson.h: jf_room_set_ir); ir_right None: a mono room; an empty
        response turns the room off"""
        left = np.ascontiguousarray(ir_left, np.float32).ravel()
        right = None if ir_right is None else np.ascontiguousarray(ir_right, np.float32).ravel()
        if right is not None and len(right) != len(left):
            raise JfError(JF_ERR_ARG, "the two ears' responses differ in length")
        self._chk(lib().jf_room_set_ir(self.h, _fp(left) if len(left) else None,
                                       _fp(right) if right is not None and len(right) else None, len(left), gain))

    @property
    def room_taps(self):
        return lib().jf_room_taps(self.h)

    def set_send(self, s, level):
        """source s sends level x its input to its bus's room, from the next processing call on (ramped over its first block)"""
        self._chk(lib().jf_source_set_send(self.h, int(s), float(level)))

    def send(self, s):
        return float(lib().jf_source_send(self.h, int(s)))

    # ---- per-source gain (include/jefferson.h: "per-source gain") ----
    def set_gain(self, s, level, fade=True):
        """source s plays at `level` (1: as without gains): reached over the next call's first block, or (fade=False) at once"""
        self._chk(lib().jf_source_set_gain(self.h, int(s), float(level), int(bool(fade))))

    def gain(self, s):
        return float(lib().jf_source_gain(self.h, int(s)))

    def set_mute(self, s, on, fade=True):
        """mute keeps the level: unmuting returns to it (jf_source_set_mute)"""
        self._chk(lib().jf_source_set_mute(self.h, int(s), int(bool(on)), int(bool(fade))))

    def muted(self, s):
        m = lib().jf_source_muted(self.h, int(s))
        if m < 0:
            raise JfError(m, "bad source index")
        return bool(m)

    def set_gains(self, levels, fade=True):
        """every source's level in one call, levels [S] (jf_sources_set_gains)"""
        levels = np.ascontiguousarray(levels, np.float32)
        assert levels.shape == (self.S,)
        self._chk(lib().jf_sources_set_gains(self.h, _fp(levels), int(bool(fade))))

    def stage_gains(self, gains):
        """effective gains [K][S] for the next process_batch* call, which must have K blocks (jf_batch_set_gains); None or
        an empty array drops a staged trajectory"""
        if gains is None or len(gains) == 0:
            self._chk(lib().jf_batch_set_gains(self.h, 0, None))
            return
        gains = np.ascontiguousarray(gains, np.float32)
        assert gains.ndim == 2 and gains.shape[1] == self.S, gains.shape
        self._chk(lib().jf_batch_set_gains(self.h, gains.shape[0], _fp(gains)))

    def profile_read_gain(self):
        """ms in desc_gain_kernel since profile_enable(2)"""
        r = C.c_double()
        self._chk(lib().jf_profile_read_gain(self.h, C.byref(r)))
        return r.value

    # ---- HRTF sets (include/jefferson.h: "HRTF sets") ----
    def add_hrtf_set(self, hrir):
        """a further set on the engine's own directions, hrir [table_rows][2][taps] -> its index (jf_engine_add_hrtf_set)"""
        hrir = np.ascontiguousarray(hrir, np.float32)
        assert hrir.ndim == 3 and hrir.shape[0] == self.table_rows() and hrir.shape[1] == 2  # the C side reads rows x 2 x taps floats
        rc = lib().jf_engine_add_hrtf_set(self.h, _fp(hrir), hrir.shape[2])
        if rc < 0:
            self._chk(rc)
        return rc

    def add_hrtf_sofa(self, path, tol_deg=0.05):
        """a further set from a SOFA file on the engine's rings -> its index (jf_engine_add_hrtf_sofa)"""
        rc = lib().jf_engine_add_hrtf_sofa(self.h, os.fsencode(path), tol_deg)
        if rc < 0:
            self._chk(rc)
        return rc

    def n_hrtf_sets(self):
        return lib().jf_num_hrtf_sets(self.h)

    def set_hrtf(self, s, hrtf_set, fade=True):
        """source s hears through `hrtf_set`: crossfaded over the next call's first block, or (fade=False) at once"""
        self._chk(lib().jf_source_set_hrtf(self.h, int(s), int(hrtf_set), int(bool(fade))))

    def hrtf_of(self, s):
        r = lib().jf_source_hrtf(self.h, int(s))
        if r < 0:
            self._chk(r)
        return r

    def set_bus_hrtf(self, bus, hrtf_set, fade=True):
        """every source that is on `bus` now (jf_bus_set_hrtf)"""
        self._chk(lib().jf_bus_set_hrtf(self.h, int(bus), int(hrtf_set), int(bool(fade))))

    def read_hrtf_set(self, hrtf_set):
        """one set's rows as read_table gives set 0's"""
        t = np.zeros((self.table_rows(), 2, self.N // 2 + 1, 2), np.float32)
        self._chk(lib().jf_debug_read_hrtf_set(self.h, int(hrtf_set), _fp(t)))
        return t.view(np.complex64)[..., 0]

    def last_set_stage(self):
        """the last run launched desc_set_kernel"""
        return bool(lib().jf_debug_last_set_stage(self.h))

    def profile_read_sets(self):
        """ms in desc_set_kernel since profile_enable(2)"""
        r = C.c_double()
        self._chk(lib().jf_profile_read_sets(self.h, C.byref(r)))
        return r.value

    # ---- bus masters (include/jefferson.h: "bus masters") ----
    def set_master(self, bus, gain, fade=True):
        """bus's master gain (1: neutral): reached over the next rendered block, or (fade=False) at once"""
        self._chk(lib().jf_bus_set_master(self.h, int(bus), float(gain), int(bool(fade))))

    def master(self, bus):
        return float(lib().jf_bus_master(self.h, int(bus)))

    def set_limiter(self, bus, ceiling, release=1.0):
        """bus's safety limiter: no sample above `ceiling` (0: off); `release`: gain regained per block, in (0, 1]"""
        self._chk(lib().jf_bus_set_limiter(self.h, int(bus), float(ceiling), float(release)))

    def limiter(self, bus):
        """(ceiling, release)"""
        c, r = np.zeros(1, np.float32), np.zeros(1, np.float32)
        self._chk(lib().jf_bus_limiter(self.h, int(bus), _fp(c), _fp(r)))
        return float(c[0]), float(r[0])

    def set_meters(self, on=True):
        self._chk(lib().jf_engine_set_meters(self.h, int(bool(on))))

    def meters(self, n_blocks=1):
        """the last rendered call's meters, [n_buses][n_blocks][4] = {peak_in, peak_out, sumsq_out, gain} (jf_bus_meters)"""
        out = np.zeros((self.n_buses, int(n_blocks), 4), np.float32)
        self._chk(lib().jf_bus_meters(self.h, int(n_blocks), _fp(out)))
        return out

    master_block = staticmethod(master_block)

    def set_lookahead(self, bus, on=True):
        """bus's limiter look-ahead: the bus is handed out one block late and the limiter's gain never steps (jf_bus_set_lookahead)"""
        self._chk(lib().jf_bus_set_lookahead(self.h, int(bus), int(bool(on))))

    def lookahead(self, bus):
        return bool(lib().jf_bus_lookahead(self.h, int(bus)))

    def bus_latency(self, bus):
        """frames by which bus's handed-out mix lags the engine: B with look-ahead latched on, else 0 (jf_bus_latency)"""
        return int(lib().jf_bus_latency(self.h, int(bus)))

    master_look_block = staticmethod(master_look_block)

    def profile_read_master(self):
        """ms in the master stage's kernels since profile_enable(2)"""
        r = C.c_double()
        self._chk(lib().jf_profile_read_master(self.h, C.byref(r)))
        return r.value

    # ---- voice gates and input meters (include/jefferson.h: "voice gates") ----
    def set_gate(self, s, open, close=None, hold_blocks=0):
        """source s's gate: opens at input peak >= `open` (0: no gate), stays open while >= `close` (default: open) and for
        `hold_blocks` blocks after (jf_source_set_gate)"""
        close = open if close is None else close
        self._chk(lib().jf_source_set_gate(self.h, int(s), float(open), float(close), int(hold_blocks)))

    def gate(self, s):
        """(open, close, hold_blocks)"""
        o, c, h = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.int32)
        self._chk(lib().jf_source_gate(self.h, int(s), _fp(o), _fp(c), _ip(h)))
        return float(o[0]), float(c[0]), int(h[0])

    def set_gates(self, open, close=None, hold_blocks=0):
        """every source the same gate (jf_sources_set_gate)"""
        close = open if close is None else close
        self._chk(lib().jf_sources_set_gate(self.h, float(open), float(close), int(hold_blocks)))

    def set_input_meters(self, on=True):
        self._chk(lib().jf_engine_set_input_meters(self.h, int(bool(on))))

    def levels(self, n_blocks=1):
        """the last rendered call's input meters, [S][n_blocks][3] = {peak, sumsq, open} (jf_source_levels)"""
        out = np.zeros((self.S, int(n_blocks), 3), np.float32)
        self._chk(lib().jf_source_levels(self.h, int(n_blocks), _fp(out)))
        return out

    gate_scan = staticmethod(gate_scan)

    def profile_read_gate(self):
        """ms in the gate stage's two kernels since profile_enable(2)"""
        r = C.c_double()
        self._chk(lib().jf_profile_read_gate(self.h, C.byref(r)))
        return r.value

    # ---- voice limits (include/jefferson.h: "voice limits") ----
    def set_voices(self, bus, max_voices, release=0.0, fade=True):
        """bus `bus` renders at most `max_voices` of its sources a block, the loudest by an envelope that falls by `release`
        per block (0: no limit) (jf_bus_set_voices)"""
        self._chk(lib().jf_bus_set_voices(self.h, int(bus), int(max_voices), float(release), int(bool(fade))))

    def voices(self, bus):
        """(max_voices, release)"""
        n, r = np.zeros(1, np.int32), np.zeros(1, np.float32)
        self._chk(lib().jf_bus_voices(self.h, int(bus), _ip(n), _fp(r)))
        return int(n[0]), float(r[0])

    def set_priority(self, s, priority):
        """0 .. 255; JF_VOICE_ALWAYS (255): always heard, takes no place (jf_source_set_priority)"""
        self._chk(lib().jf_source_set_priority(self.h, int(s), int(priority)))

    def priority(self, s):
        r = lib().jf_source_priority(self.h, int(s))
        if r < 0:
            raise JfError(r, "priority")
        return r

    def heard(self, n_blocks=1):
        """the last rendered call's voices, [S][n_blocks][2] = {env, keep} (jf_source_heard)"""
        out = np.zeros((self.S, int(n_blocks), 2), np.float32)
        self._chk(lib().jf_source_heard(self.h, int(n_blocks), _fp(out)))
        return out

    voice_select = staticmethod(voice_select)

    def profile_read_voices(self):
        """ms in the voice limits' two kernels since profile_enable(2)"""
        r = C.c_double()
        self._chk(lib().jf_profile_read_voices(self.h, C.byref(r)))
        return r.value

    # ---- talker levelling (include/jefferson.h: "talker levelling") ----
    def set_leveller(self, s, target, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0):
        """source s is levelled towards the linear peak `target` (0: off): frozen below `floor`, within min_gain .. max_gain, by at
        most `fall` / `rise` a block (jf_source_set_leveller)"""
        self._chk(lib().jf_source_set_leveller(self.h, int(s), _fp(_leveller(target, floor, min_gain, max_gain, fall, rise))))

    def set_levellers(self, target, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0):
        """every source (jf_sources_set_leveller)"""
        self._chk(lib().jf_sources_set_leveller(self.h, _fp(_leveller(target, floor, min_gain, max_gain, fall, rise))))

    def leveller(self, s):
        """dict(target, floor, min_gain, max_gain, fall, rise); target is 0 before anything was set"""
        out = np.zeros(6, np.float32)
        self._chk(lib().jf_source_leveller(self.h, int(s), _fp(out)))
        return dict(zip(LEVELLER_FIELDS, (float(v) for v in out)))

    def level_gains(self, n_blocks=1):
        """the last rendered call's levelling gains a[k], [S][n_blocks] (jf_source_level_gains)"""
        out = np.zeros((self.S, int(n_blocks)), np.float32)
        self._chk(lib().jf_source_level_gains(self.h, int(n_blocks), _fp(out)))
        return out

    level_scan = staticmethod(level_scan)

    def profile_read_level(self):
        """ms in level_scan_kernel since profile_enable(2)"""
        r = C.c_double()
        self._chk(lib().jf_profile_read_level(self.h, C.byref(r)))
        return r.value

    # ---- hearing range (include/jefferson.h: "hearing range") ----
    def set_range(self, bus, near, far):
        """the listener of `bus` hears talkers within `near` in full and none beyond `far` (far = 0: off) (jf_bus_set_range)"""
        self._chk(lib().jf_bus_set_range(self.h, int(bus), float(near), float(far)))

    def range(self, bus):
        """(near, far); both 0 before anything was set (jf_bus_range)"""
        a, b = np.zeros(1, np.float32), np.zeros(1, np.float32)
        self._chk(lib().jf_bus_range(self.h, int(bus), _fp(a), _fp(b)))
        return float(a[0]), float(b[0])

    def set_range_exempt(self, s, on=True):
        """source s is heard at any distance (jf_source_set_range_exempt)"""
        self._chk(lib().jf_source_set_range_exempt(self.h, int(s), 1 if on else 0))

    def range_exempt(self, s):
        rc = lib().jf_source_range_exempt(self.h, int(s))
        if rc < 0:
            self._chk(rc)
        return bool(rc)

    def range_gains(self, n_blocks=1):
        """the last rendered call's hearing-range gains h[k], [S][n_blocks] (jf_source_range_gains)"""
        out = np.zeros((self.S, int(n_blocks)), np.float32)
        self._chk(lib().jf_source_range_gains(self.h, int(n_blocks), _fp(out)))
        return out

    range_scan = staticmethod(range_scan)

    def range_bytes(self):
        """device and pinned memory held for ranges (0 until a call is latched with one)"""
        return int(lib().jf_debug_range_bytes(self.h))

    def profile_read_range(self):
        """ms in range_gain_kernel since profile_enable(2)"""
        r = C.c_double()
        self._chk(lib().jf_profile_read_range(self.h, C.byref(r)))
        return r.value

    def room_wet(self, n_blocks):
        """the room's wet contribution to the last processing call, [n_buses][n_blocks][2B] (jefferson_debug.h)"""
        out = np.zeros((self.n_buses, int(n_blocks), 2 * self.B), np.float32)
        self._chk(lib().jf_debug_room_wet(self.h, int(n_blocks), _fp(out)))
        return out

    def _out(self, *shape):
        """zeros of a call's output shape, behind a bus axis when the engine has more than one bus"""
        nb = self.n_buses
        return np.zeros(shape if nb == 1 else (nb,) + shape, np.float32)

    def _inp(self, inp, n):
        """[n_live][n] float32 for the *_in calls"""
        inp = np.ascontiguousarray(inp, np.float32).reshape(-1, n)
        assert inp.shape[0] == self.n_live(), (inp.shape, self.n_live())
        return inp

    def process_block(self, inp=None):
        out = self._out(2 * self.B)
        if inp is None:
            self._chk(lib().jf_process_block(self.h, _fp(out)))
        else:
            inp = self._inp(inp, self.B)
            self._chk(lib().jf_process_block_in(self.h, _fp(inp), _fp(out)))
        return out

    def submit_block(self, inp=None):
        if inp is None:
            return lib().jf_submit_block(self.h)
        inp = self._inp(inp, self.B)
        return lib().jf_submit_block_in(self.h, _fp(inp))

    def collect_block(self):
        out = self._out(2 * self.B)
        rc = lib().jf_collect_block(self.h, _fp(out))
        return rc, out

    def callback(self, inp=None):
        out = self._out(2 * self.B)
        if inp is None:
            self._chk(lib().jf_callback(self.h, _fp(out)))
        else:
            inp = self._inp(inp, self.B)
            self._chk(lib().jf_callback_in(self.h, _fp(inp), _fp(out)))
        return out

    def pa_callback(self, inp=None):
        """jf_pa_callback as PortAudio calls it; inp: interleaved [B][n_live] or None (a stream without input).
        With more than one bus: [B][2 n_buses], the stream's interleaved output channels."""
        nb = self.n_buses
        out = np.zeros(2 * self.B, np.float32) if nb == 1 else np.zeros((self.B, 2 * nb), np.float32)
        if inp is not None:
            inp = np.ascontiguousarray(inp, np.float32)
            assert inp.size == self.B * self.n_live()
        lib().jf_pa_callback(None if inp is None else inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), self.B,
                             None, 0, self.h)
        return out

    def set_mode(self, mode):
        self._chk(lib().jf_set_mode(self.h, int(mode)))

    def set_pause(self, p):
        self._chk(lib().jf_set_pause(self.h, int(p)))

    def process_batch(self, pos, inp=None):
        pos = np.ascontiguousarray(pos, np.float32)
        K, S = pos.shape[0], pos.shape[1]
        assert S == self.S and pos.shape[2] == 5
        mix = self._out(K, 2 * self.B)
        if inp is None:
            self._chk(lib().jf_process_batch(self.h, K, _fp(pos), _fp(mix)))
        else:
            inp = self._inp(inp, K * self.B)
            self._chk(lib().jf_process_batch_in(self.h, K, _fp(inp), _fp(pos), _fp(mix)))
        return mix

    def set_listener(self, bus, position, orientation):
        """bus's listener: head centre `position` and unit quaternion `orientation` {qw, qx, qy, qz}, head -> world
        (include/jefferson.h: jf_listener_set_pose)"""
        p = np.ascontiguousarray(position, np.float32)
        q = np.ascontiguousarray(orientation, np.float32)
        assert p.shape == (3,) and q.shape == (4,)
        self._chk(lib().jf_listener_set_pose(self.h, int(bus), _fp(p), _fp(q)))

    def listener(self, bus):
        o = np.zeros(7, np.float32)
        self._chk(lib().jf_listener_get_pose(self.h, int(bus), _fp(o)))
        return o

    def set_world(self, s, x, y, z):
        """source s at a world position: heard as its bus's listener hears it (jf_source_set_world)"""
        self._chk(lib().jf_source_set_world(self.h, int(s), x, y, z))

    def world(self, s):
        o = np.zeros(3, np.float32)
        self._chk(lib().jf_source_get_world(self.h, int(s), _fp(o)))
        return o

    def _world_args(self, world, poses):
        world = np.ascontiguousarray(world, np.float32)
        poses = np.ascontiguousarray(poses, np.float32)
        K = world.shape[0]
        assert world.shape == (K, self.S, 3) and poses.shape == (K, self.n_buses, 7), (world.shape, poses.shape)
        return K, world, poses

    def process_batch_world(self, world, poses, inp=None):
        """world [K][S][3], poses [K][n_buses][7] -> the mix of K blocks (jf_process_batch_world)"""
        K, world, poses = self._world_args(world, poses)
        mix = self._out(K, 2 * self.B)
        inp = None if inp is None else self._inp(inp, K * self.B)
        self._chk(lib().jf_process_batch_world(self.h, K, None if inp is None else _fp(inp), _fp(world), _fp(poses), _fp(mix)))
        return mix

    def upload_world(self, world, poses):
        """upload_positions for a trajectory of world positions and poses (jf_batch_upload_world)"""
        K, world, poses = self._world_args(world, poses)
        self._chk(lib().jf_batch_upload_world(self.h, K, _fp(world), _fp(poses)))

    def pose_device(self, bus, world, poses):
        """pose_kernel alone: bus [S] (or None), world [K][S][3], poses [K][n_buses][7] -> records [K][S][5]
        (jefferson_debug.h: jf_debug_pose_device; the sizes are the arrays', not the engine's)"""
        world = np.ascontiguousarray(world, np.float32)
        poses = np.ascontiguousarray(poses, np.float32)
        K, S, nb = world.shape[0], world.shape[1], poses.shape[1]
        assert world.shape == (K, S, 3) and poses.shape == (K, nb, 7)
        bus = None if bus is None else np.ascontiguousarray(bus, np.int32)
        assert bus is None or bus.shape == (S,)
        out = np.zeros((K, S, 5), np.float32)
        self._chk(lib().jf_debug_pose_device(self.h, K, S, nb, None if bus is None else _ip(bus), _fp(world), _fp(poses), _fp(out)))
        return out

    # ---- objects (include/jefferson.h: "objects") ----
    def set_objects(self, n):
        self._chk(lib().jf_engine_set_objects(self.h, int(n)))

    @property
    def n_objects(self):
        return int(lib().jf_num_objects(self.h))

    def set_object(self, s, obj):
        """attach source s to object obj; obj < 0 detaches (jf_source_set_object)"""
        self._chk(lib().jf_source_set_object(self.h, int(s), int(obj)))

    def object_of(self, s):
        """the object source s is attached to, -1: none"""
        return int(lib().jf_source_object(self.h, int(s)))

    def set_object_world(self, obj, x, y, z):
        self._chk(lib().jf_object_set_world(self.h, int(obj), x, y, z))

    def object_world(self, obj):
        o = np.zeros(3, np.float32)
        self._chk(lib().jf_object_get_world(self.h, int(obj), _fp(o)))
        return o

    def _object_args(self, objects, poses):
        objects = np.ascontiguousarray(objects, np.float32)
        poses = np.ascontiguousarray(poses, np.float32)
        K = objects.shape[0]
        assert objects.shape == (K, self.n_objects, 3) and poses.shape == (K, self.n_buses, 7), (objects.shape, poses.shape)
        return K, objects, poses

    def process_batch_objects(self, objects, poses, inp=None):
        """objects [K][n_objects][3], poses [K][n_buses][7] -> the mix of K blocks (jf_process_batch_objects)"""
        K, objects, poses = self._object_args(objects, poses)
        mix = self._out(K, 2 * self.B)
        inp = None if inp is None else self._inp(inp, K * self.B)
        self._chk(lib().jf_process_batch_objects(self.h, K, None if inp is None else _fp(inp), _fp(objects), _fp(poses), _fp(mix)))
        return mix

    def upload_objects(self, objects, poses):
        """upload_world for a trajectory of object positions and poses (jf_batch_upload_objects)"""
        K, objects, poses = self._object_args(objects, poses)
        self._chk(lib().jf_batch_upload_objects(self.h, K, _fp(objects), _fp(poses)))

    # ---- object poses, following listeners, talker cones (include/jefferson.h: "talker cones and heads that follow objects") ----
    def set_object_pose(self, obj, position, orientation):
        """object obj at `position`, facing along the unit quaternion `orientation` {qw, qx, qy, qz} (jf_object_set_pose)"""
        p = np.ascontiguousarray(position, np.float32)
        q = np.ascontiguousarray(orientation, np.float32)
        assert p.shape == (3,) and q.shape == (4,)
        self._chk(lib().jf_object_set_pose(self.h, int(obj), _fp(p), _fp(q)))

    def object_pose(self, obj):
        o = np.zeros(7, np.float32)
        self._chk(lib().jf_object_get_pose(self.h, int(obj), _fp(o)))
        return o

    def follow_object(self, bus, obj):
        """the listener of `bus` is object obj from the next block on; obj < 0 detaches (jf_listener_follow_object)"""
        self._chk(lib().jf_listener_follow_object(self.h, int(bus), int(obj)))

    def listener_object(self, bus):
        """the object the listener of `bus` follows, -1: none"""
        return int(lib().jf_listener_object(self.h, int(bus)))

    def set_cone(self, obj, inner, outer, outer_gain):
        """object obj talks into a cone: full level within `inner` degrees, `outer_gain` beyond `outer` (jf_object_set_cone)"""
        self._chk(lib().jf_object_set_cone(self.h, int(obj), float(inner), float(outer), float(outer_gain)))

    def cone(self, obj):
        """(inner, outer, outer_gain); (360, 360, 1) before anything was set (jf_object_cone)"""
        a, b, c = (np.zeros(1, np.float32) for _ in range(3))
        self._chk(lib().jf_object_cone(self.h, int(obj), _fp(a), _fp(b), _fp(c)))
        return float(a[0]), float(b[0]), float(c[0])

    def cone_gains(self, n_blocks=1):
        """the last rendered call's cone gains d[k], [S][n_blocks] (jf_source_cone_gains)"""
        out = np.zeros((self.S, int(n_blocks)), np.float32)
        self._chk(lib().jf_source_cone_gains(self.h, int(n_blocks), _fp(out)))
        return out

    cone_scan = staticmethod(cone_scan)

    def cone_bytes(self):
        """device and pinned memory held for cones (0 until a call is latched with one)"""
        return int(lib().jf_debug_cone_bytes(self.h))

    def profile_read_cone(self):
        """ms in cone_gain_kernel since profile_enable(2)"""
        r = C.c_double(0.0)
        self._chk(lib().jf_profile_read_cone(self.h, C.byref(r)))
        return r.value

    def _object_pose_args(self, object_poses, listener_poses):
        object_poses = np.ascontiguousarray(object_poses, np.float32)
        K = object_poses.shape[0]
        assert object_poses.shape == (K, self.n_objects, 7), object_poses.shape
        if listener_poses is not None:
            listener_poses = np.ascontiguousarray(listener_poses, np.float32)
            assert listener_poses.shape == (K, self.n_buses, 7), listener_poses.shape
        return K, object_poses, listener_poses

    def process_batch_poses(self, object_poses, listener_poses=None, inp=None):
        """object_poses [K][n_objects][7], listener_poses [K][n_buses][7] or None (every bus follows an object) -> the mix of K
        blocks (jf_process_batch_poses)"""
        K, op, lp = self._object_pose_args(object_poses, listener_poses)
        mix = self._out(K, 2 * self.B)
        inp = None if inp is None else self._inp(inp, K * self.B)
        self._chk(lib().jf_process_batch_poses(self.h, K, None if inp is None else _fp(inp), _fp(op), None if lp is None else _fp(lp),
                                               _fp(mix)))
        return mix

    def upload_object_poses(self, object_poses, listener_poses=None):
        """upload_objects for a trajectory of object poses (jf_batch_upload_object_poses)"""
        K, op, lp = self._object_pose_args(object_poses, listener_poses)
        self._chk(lib().jf_batch_upload_object_poses(self.h, K, _fp(op), None if lp is None else _fp(lp)))

    def pose_objects_device(self, bus, object_of, objects, poses):
        """pose_object_kernel alone: bus [S] (or None), object_of [S], objects [K][n_obj][3], poses [K][n_buses][7] -> records
        [K][S][5] (jefferson_debug.h: jf_debug_pose_objects_device; the sizes are the arrays', not the engine's)"""
        objects = np.ascontiguousarray(objects, np.float32)
        poses = np.ascontiguousarray(poses, np.float32)
        object_of = np.ascontiguousarray(object_of, np.int32)
        K, no, nb, S = objects.shape[0], objects.shape[1], poses.shape[1], object_of.shape[0]
        assert objects.shape == (K, no, 3) and poses.shape == (K, nb, 7) and object_of.shape == (S,)
        bus = None if bus is None else np.ascontiguousarray(bus, np.int32)
        assert bus is None or bus.shape == (S,)
        out = np.zeros((K, S, 5), np.float32)
        self._chk(lib().jf_debug_pose_objects_device(self.h, K, S, nb, no, None if bus is None else _ip(bus), _ip(object_of),
                                                     _fp(objects), _fp(poses), _fp(out)))
        return out

    def profile_read_pose(self):
        """(ms in pose_kernel and pose_object_kernel, launches) since profile_enable(2)"""
        ms, n = C.c_double(), C.c_long()
        self._chk(lib().jf_profile_read_pose(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def pose_device_bytes(self):
        """device memory held for listener poses and objects (0 before the first world / objects batch call)"""
        return int(lib().jf_debug_pose_device_bytes(self.h))

    def set_latched(self, records):
        """every source's position := its latched record [S][5] (what S setter calls leave behind)"""
        records = np.ascontiguousarray(records, np.float32)
        assert records.shape == (self.S, 5)
        self._chk(lib().jf_sources_set_latched(self.h, _fp(records)))

    def upload_positions(self, pos):
        pos = np.ascontiguousarray(pos, np.float32)
        assert pos.shape[1] == self.S and pos.shape[2] == 5
        self._chk(lib().jf_batch_upload_positions(self.h, pos.shape[0], _fp(pos)))

    def batch_run(self, first, n, d_out=None):
        self._chk(lib().jf_batch_run(self.h, first, n, d_out))

    def synchronize(self):
        self._chk(lib().jf_synchronize(self.h))

    def batch_fetch(self, n_blocks):
        """the engine's own mix of the last batch_run (d_out_mix = NULL), [n_blocks][2B], on the host"""
        out = self._out(int(n_blocks), 2 * self.B)
        self._chk(lib().jf_batch_fetch(self.h, int(n_blocks), _fp(out)))
        return out

    def mix_device_ptr(self):
        return lib().jf_batch_mix_device(self.h)

    def partial_device_ptr(self):
        return lib().jf_batch_partial_device(self.h)

    def stream_ptr(self):
        return lib().jf_engine_stream(self.h)

    def profile_enable(self, on):
        self._chk(lib().jf_profile_enable(self.h, int(on)))

    def profile_set_stride(self, every):
        self._chk(lib().jf_profile_set_stride(self.h, int(every)))

    def profile_read(self):
        f, p, m = C.c_double(), C.c_double(), C.c_double()
        n = C.c_long()
        self._chk(lib().jf_profile_read(self.h, C.byref(f), C.byref(p), C.byref(m), C.byref(n)))
        return {"fused_ms": f.value, "prep_ms": p.value, "mix_ms": m.value, "launches": n.value}

    def set_reverb(self, ir, gain=1.0):
        ir = np.ascontiguousarray(ir, np.float32)
        self._chk(lib().jf_reverb_set_ir(self.h, _fp(ir) if len(ir) else None, len(ir), gain))

    def profile_read_reverb(self):
        r = C.c_double()
        self._chk(lib().jf_profile_read_reverb(self.h, C.byref(r)))
        return r.value

    def profile_read_spectrum(self):
        """ms in shared_spectrum_kernel since profile_enable(2) (part of profile_read()'s fused_ms too)"""
        r = C.c_double()
        self._chk(lib().jf_profile_read_spectrum(self.h, C.byref(r)))
        return r.value

    def set_source_group(self, g):
        self._chk(lib().jf_debug_set_source_group(self.h, int(g)))

    def last_kernels(self):
        return lib().jf_debug_last_kernels(self.h).decode().split(";")

    def read_stamps(self, n):
        out = np.zeros(n, np.uint64)
        self._chk(lib().jf_debug_read_stamps(self.h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), n))
        return out

    def source_order(self):
        o = np.zeros(self.S, np.int32)
        self._chk(lib().jf_debug_source_order(self.h, _ip(o)))
        return o

    def last_source_group(self):
        return lib().jf_debug_last_source_group(self.h)

    def set_grid_limit(self, wgs):
        self._chk(lib().jf_debug_set_grid_limit(self.h, int(wgs)))

    def set_prep_ahead(self, on):
        self._chk(lib().jf_debug_set_prep_ahead(self.h, int(bool(on))))

    def last_block_peak(self):
        return float(lib().jf_last_block_peak(self.h))

    def stage_taps(self, positions, windows=None):
        """positions [n][5] (and windows [n][1024]) -> D [n][513] complex64 (and Y [n][2][513] complex64)."""
        positions = np.ascontiguousarray(positions, np.float32)
        n = positions.shape[0]
        dist = np.zeros((n, NC, 2), np.float32)
        spec = None
        if windows is not None:
            windows = np.ascontiguousarray(windows, np.float32)
            assert windows.shape == (n, PAD_LEN)
            spec = np.zeros((n, 2, NC, 2), np.float32)
        self._chk(lib().jf_debug_stage_taps(self.h, n, _fp(positions), _fp(windows) if spec is not None else None,
                                            _fp(dist), _fp(spec) if spec is not None else None))
        d = dist.view(np.complex64)[..., 0]
        return d if spec is None else (d, spec.view(np.complex64)[..., 0])

    def set_reverb_partitioning(self, how):
        """0 by length, 1 uniform, 2 non-uniform; in effect from the next set_reverb"""
        self._chk(lib().jf_debug_set_reverb_partitioning(self.h, int(how)))

    def set_reverb_async(self, on):
        """one-block calls: the big partitions' kernels on a second stream (default) or in line"""
        self._chk(lib().jf_debug_set_reverb_async(self.h, int(bool(on))))

    def set_reverb_ahead(self, on):
        """one-block calls launch the next block's reverb stage behind their own spatialiser (default) or not"""
        self._chk(lib().jf_debug_set_reverb_ahead(self.h, int(bool(on))))

    def reverb_ahead_pending(self):
        """the next block's reverb stage has been launched ahead and is still pending"""
        return bool(lib().jf_debug_reverb_ahead_pending(self.h))

    def set_reverb_side_workgroups(self, n):
        """workgroups of the product kernel on the reverb's side stream (tuning runs)"""
        self._chk(lib().jf_debug_set_reverb_side_workgroups(self.h, int(n)))

    def set_reverb_lazy_state(self, on):
        """batch calls of whole big blocks put the small transforms of their last blocks off (default) or form them at once"""
        self._chk(lib().jf_debug_set_reverb_lazy_state(self.h, int(bool(on))))

    def set_reverb_head_fused(self, on):
        """one-block calls: the reverb's head inside the real-time kernel's launch, or as a kernel of its own (default: measured 5 us
        faster per block)"""
        self._chk(lib().jf_debug_set_reverb_head_fused(self.h, int(bool(on))))

    def reverb_partitions(self):
        """(partitions of B the response has, head partitions in use, big partitions, taps per big partition)"""
        h, b, t = C.c_int(), C.c_int(), C.c_int()
        n = lib().jf_debug_reverb_partitions(self.h, C.byref(h), C.byref(b), C.byref(t))
        return n, h.value, b.value, t.value

    def set_reverb_form(self, form):
        self._chk(lib().jf_debug_set_reverb_form(self.h, int(form)))

    def read_device(self, ptr, shape):
        out = np.zeros(shape, np.float32)
        self._chk(lib().jf_debug_copy_from_device(self.h, ptr, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def set_rt_max_sources(self, n):
        self._chk(lib().jf_debug_set_rt_max_sources(self.h, int(n)))

    def table_rows(self):
        return lib().jf_table_rows(self.h)

    def read_table(self):
        t = np.zeros((self.table_rows(), 2, self.N // 2 + 1, 2), np.float32)  # Nc bins per ear
        self._chk(lib().jf_debug_read_table(self.h, _fp(t)))
        return t.view(np.complex64)[..., 0]

    def set_interp_table(self, on):
        """0 / False = never, 1 / True = always, 2 = decided per run (default)"""
        self._chk(lib().jf_debug_set_interp_table(self.h, int(on)))

    def last_run_used_rows(self):
        return bool(lib().jf_debug_last_run_used_rows(self.h))

    def interp_table(self):
        """0 = off / not built, 1 = always, 2 = decided per run"""
        return lib().jf_debug_interp_table(self.h)

    def interp_table_built(self):
        """the engine holds the 47 160 pre-interpolated rows (built by the first run that takes them)"""
        return bool(lib().jf_debug_interp_table_built(self.h))

    def count_desc_flags(self, n_items, mask):
        n = lib().jf_debug_count_desc_flags(self.h, int(n_items), int(mask))
        if n < 0:
            self._chk(n)
        return n

    def read_table_rows(self, first_row, n):
        """n rows in the device layout: [n][N/2][4] = {L.re, L.im, R.re, R.im} (bin 0: {L[0], L[N/2], R[0], R[N/2]})."""
        t = np.zeros((n, self.N // 2, 4), np.float32)
        self._chk(lib().jf_debug_read_table_rows(self.h, int(first_row), int(n), _fp(t)))
        return t

    def interp_device(self, ele, azi):
        ele = np.ascontiguousarray(ele, np.float32)
        azi = np.ascontiguousarray(azi, np.float32)
        n = len(ele)
        rows = np.zeros((n, 4), np.int32)
        w = np.zeros((n, 4), np.float32)
        nt = np.zeros(n, np.int32)
        self._chk(lib().jf_debug_interp_device(self.h, n, _fp(ele), _fp(azi), _ip(rows), _fp(w), _ip(nt)))
        return rows, w, nt

    def rfft_device(self, windows):
        windows = np.ascontiguousarray(windows, np.float32)
        n = windows.shape[0]
        assert windows.shape[1] == self.N  # the engine's PAD_LEN (1024 or 2048)
        sp = np.zeros((n, self.N // 2 + 1, 2), np.float32)
        self._chk(lib().jf_debug_rfft_device(self.h, n, _fp(windows), _fp(sp)))
        return sp.view(np.complex64)[..., 0]
