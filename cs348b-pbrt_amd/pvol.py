"""ctypes binding of libpvol.so, the C ABI declared in include/pvol.h.

This is plumbing only: every compute call goes to the HIP library, and loading fails loudly when
the library has not been built (there is no Python or CPU fallback).
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PVOL_LIB") or os.path.join(_HERE, "libpvol.so")  # PVOL_LIB: A/B builds of the same ABI

_f32p = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)


class PvolError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        RuntimeError.__init__(self, "%s: %s (%d)" % (where, lib().pvol_strerror(status).decode(), status))


# pvol_shoot_comm: how the ranks of pvol_preprocess_ranks exchange data (exactly one of nccl_comm / allgather set)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)


class ShootComm(C.Structure):
    _fields_ = [("nccl_comm", C.c_void_p), ("allgather", ALLGATHER_FN), ("user", C.c_void_p)]


# ---- final gather, sampling half (include/pvol.h: pvol_gather_*)
GATHER_K = 50   # nIndirSamplePhotons (integrators/photonmap.cpp:190)
# pvol_gather_sample
GATHER_SAMPLE_DTYPE = np.dtype([("wi", "<f4", 3), ("weight", "<f4"), ("bsdf_pdf", "<f4"), ("photon_pdf", "<f4"), ("photon_index", "<u4"), ("valid", "<u4")])
# GatherNode (csrc/pvol_gather_tree.h), what the test hook pvol_gather_tree_build fills
GATHER_NODE_DTYPE = np.dtype([("p", "<f4", 3), ("split_pos", "<f4"), ("split_axis", "<u4"), ("has_left_child", "<u4"), ("right_child", "<u4"),
                              ("index", "<u4")])
# pvol_gather_ray (final gather, tracing half: pvol_final_gather*)
GATHER_RAY_DTYPE = np.dtype([("t", "<f4"), ("n_gather", "<f4", 3), ("radiance_index", "<u4"), ("prim", "<i4"), ("hit", "<u4"), ("drew", "<u4")])
GATHER_NONE = 0xffffffff
assert GATHER_SAMPLE_DTYPE.itemsize == 32 and GATHER_NODE_DTYPE.itemsize == 32 and GATHER_RAY_DTYPE.itemsize == 32


class GatherCheck(C.Structure):   # the arguments pvol_check_gather judges (csrc/pvol_host.h)
    _fields_ = [("indirect", C.POINTER(abi.PhotonArray)), ("p", _f32p), ("count", C.c_uint32), ("max_dist", C.c_float),
                ("out_index", C.c_void_p), ("out_d2", C.c_void_p), ("out_found", C.c_void_p), ("out_rounds", C.c_void_p),
                ("frames", _f32p), ("wo", _f32p), ("u_bsdf", _f32p), ("u_photon", _f32p), ("n_samples", C.c_int32), ("cos_gather_angle", C.c_float),
                ("out_bsdf", C.c_void_p), ("out_photon", C.c_void_p)]


class FinalGatherCheck(C.Structure):   # the arguments pvol_check_final_gather judges (csrc/pvol_host.h)
    _fields_ = [("p", _f32p), ("frames", _f32p), ("wo", _f32p), ("kd", _f32p), ("ray_eps", _f32p), ("count", C.c_uint32), ("max_dist", C.c_float),
                ("n_samples", C.c_int32), ("cos_gather_angle", C.c_float), ("u_bsdf", _f32p), ("u_photon", _f32p), ("L", C.c_void_p),
                ("draws", C.c_void_p)]


def gather_cos_angle(gather_angle):
    """PhotonShooter's cosGatherAngle for a "gatherangle" in degrees (core/photonshooter.cpp:413): Radians() in fp32, cos in double,
    the result stored as a float."""
    rad = np.float32(np.float32(np.float32(3.14159265358979323846) / np.float32(180.0)) * np.float32(gather_angle))
    return float(np.float32(np.cos(np.float64(rad))))


def gather_tree(p):
    """The gather map's kd-tree over p[n,3] as the host builds it (pvol_gather_tree_build; no GPU): (nodes, depth), nodes a
    GATHER_NODE_DTYPE array in the reference's node numbering."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1)
    n = p.size // 3
    nodes, depth = np.zeros(n, GATHER_NODE_DTYPE), C.c_int32()
    _check(lib().pvol_gather_tree_build(p.ctypes.data_as(_f32p), n, nodes.ctypes.data, C.byref(depth)), "pvol_gather_tree_build")
    return nodes, depth.value


def gloo_allgather(group=None):
    """A host all-gather for PhotonVolume.preprocess_ranks over torch.distributed (gloo: CPU tensors): bytes -> list of bytes,
    one entry per rank in rank order."""
    import torch
    import torch.distributed as dist

    def allgather(data):
        n = dist.get_world_size(group)
        if not data:
            return [b""] * n
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        out = [torch.empty_like(t) for _ in range(n)]
        dist.all_gather(out, t, group=group)
        return [o.numpy().tobytes() for o in out]
    return allgather


_lib = None


def lib():
    """Load libpvol.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no fallback path" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.pvol_abi_version.restype = C.c_int
        L.pvol_strerror.restype = C.c_char_p
        L.pvol_strerror.argtypes = [C.c_int]
        L.pvol_device_count.restype = C.c_int
        L.pvol_default_params.argtypes = [C.POINTER(abi.Params)]
        L.pvol_default_params.restype = None
        L.pvol_create.argtypes = [C.POINTER(abi.Params), C.POINTER(C.c_void_p)]
        L.pvol_destroy.argtypes = [C.c_void_p]
        L.pvol_destroy.restype = None
        L.pvol_set_scene.argtypes = [C.c_void_p, C.POINTER(abi.Scene)]
        L.pvol_set_triangle_normals.argtypes = [C.c_void_p, _f32p, C.c_uint32]
        L.pvol_check_triangle_normals.argtypes = [C.POINTER(abi.Scene), _f32p, C.c_uint32]
        L.pvol_upload_photons.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, C.c_uint32]
        L.pvol_preprocess.argtypes = [C.c_void_p, C.c_uint32]
        L.pvol_preprocess_blocks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.pvol_preprocess_ranks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShootComm)]
        L.pvol_get_exchange_seconds.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.pvol_photon_count.argtypes = [C.c_void_p, _u32p]
        L.pvol_download_photons.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, C.c_uint32]
        L.pvol_li_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, _f32p, _u32p]
        L.pvol_li_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        L.pvol_li.argtypes = [C.c_void_p, C.c_void_p, _u32p, C.POINTER(C.c_int32), _f32p, _f32p]
        L.pvol_li_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, _u32p, C.POINTER(C.c_int32), _f32p, _f32p, C.POINTER(C.c_int32)]
        L.pvol_set_li_coalescing.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.pvol_get_li_coalescing_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.pvol_transmittance_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _f32p]
        L.pvol_get_stats.argtypes = [C.c_void_p, C.POINTER(abi.Stats), C.c_int]
        L.pvol_enable_stats.argtypes = [C.c_void_p, C.c_int]
        L.pvol_set_volume_integrator.argtypes = [C.c_void_p, C.c_int]
        L.pvol_get_volume_integrator.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.pvol_single_plan.argtypes = [C.POINTER(abi.SinglePlanIn), C.POINTER(abi.SinglePlan)]
        L.pvol_single_plan.restype = None
        L.pvol_single_roulette_possible.argtypes = [C.c_int, C.c_double, C.c_float, C.c_float]
        L.pvol_kernel_time_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.pvol_get_shoot_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.pvol_march_kernel_name.argtypes = [C.c_void_p]
        L.pvol_check_errors.argtypes = [C.c_void_p]
        L.pvol_get_preprocess_seconds.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.pvol_get_accel_info.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.pvol_surface_photon_count.argtypes = [C.c_void_p, C.c_int, _u32p, _u32p]
        L.pvol_download_surface_photons.argtypes = [C.c_void_p, C.c_int, _f32p, _f32p, _f32p, C.c_uint32]
        L.pvol_radiance_photon_count.argtypes = [C.c_void_p, _u32p]
        L.pvol_download_radiance_photons.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, _f32p, C.c_uint32]
        L.pvol_compute_radiance.argtypes = [C.c_void_p, C.c_int32, C.c_float]
        L.pvol_compute_radiance_arrays.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.POINTER(C.POINTER(abi.PhotonArray)), _f32p, _f32p, _f32p, _f32p,
                                                   C.c_uint32]
        L.pvol_radiance_lo_count.argtypes = [C.c_void_p, _u32p]
        L.pvol_download_radiance_lo.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, C.c_uint32]
        L.pvol_radiance_lookup.argtypes = [C.c_void_p, _f32p, _f32p, C.c_uint32, _f32p, _u32p]
        L.pvol_radiance_lookup_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pvol_check_radiance.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int32, C.c_float, C.POINTER(C.POINTER(abi.PhotonArray)), _f32p, _f32p, _f32p,
                                          _f32p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]
        L.pvol_build_gather_map.argtypes = [C.c_void_p]
        L.pvol_build_gather_map_arrays.argtypes = [C.c_void_p, C.POINTER(abi.PhotonArray)]
        L.pvol_gather_map_count.argtypes = [C.c_void_p, _u32p]
        L.pvol_gather_photons.argtypes = [C.c_void_p, _f32p, C.c_uint32, C.c_float, _u32p, _f32p, _u32p, _u32p]
        L.pvol_gather_photons_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pvol_gather_directions.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, C.c_uint32, C.c_float, C.c_int32, C.c_float, _f32p, _f32p, C.c_void_p,
                                             C.c_void_p]
        L.pvol_gather_directions_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_float,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pvol_gather_tree_build.argtypes = [_f32p, C.c_uint32, C.c_void_p, C.POINTER(C.c_int32)]
        L.pvol_check_gather.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(GatherCheck), C.c_int]
        L.pvol_final_gather.argtypes = [C.c_void_p, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_uint32, C.c_float, C.c_int32, C.c_float, _f32p, _f32p,
                                        _f32p, _u32p, C.c_void_p, C.c_void_p]
        L.pvol_final_gather_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint32, C.c_float, C.c_int32, C.c_float] + [C.c_void_p] * 7
        L.pvol_check_final_gather.argtypes = [C.c_int, C.POINTER(FinalGatherCheck), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]
        L.pvol_final_gather_slice.argtypes = [C.c_int32, C.c_uint64]
        L.pvol_final_gather_slice.restype = C.c_uint32
        L.pvol_final_gather_set_scratch_bound.argtypes = [C.c_void_p, C.c_uint64]
        L.pvol_lphoton_batch.argtypes = [C.c_void_p, _f32p, _f32p, C.c_uint32, C.c_int, _f32p, _u32p, _f32p]
        L.pvol_lphoton_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pvol_check_lphoton.argtypes = [C.c_int, C.POINTER(abi.LPhotonCheck), C.c_int, C.c_float]
        L.pvol_lphoton_slice.argtypes = [C.c_uint64]
        L.pvol_lphoton_slice.restype = C.c_uint32
        L.pvol_lphoton_set_scratch_bound.argtypes = [C.c_void_p, C.c_uint64]
        L.pvol_radiance_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(abi.RadianceOut)]
        L.pvol_radiance_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(abi.RadianceOut), C.c_void_p]
        L.pvol_radiance_batch_check.argtypes = [C.c_int, C.POINTER(abi.RadianceBatchCheck), C.c_int, C.c_int, C.c_int]
        L.pvol_radiance_slice.argtypes = [C.c_uint32, C.c_uint64]
        L.pvol_radiance_slice.restype = C.c_uint32
        L.pvol_radiance_slice_cut.argtypes = [_u32p, C.c_uint32, C.c_uint64]
        L.pvol_radiance_slice_cut.restype = C.c_uint32
        L.pvol_radiance_slice_streams.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, C.c_void_p, _u32p, _u32p]
        L.pvol_radiance_max_segments.argtypes = [C.c_int, C.c_int32]
        L.pvol_radiance_max_segments.restype = C.c_uint32
        L.pvol_radiance_set_scratch_bound.argtypes = [C.c_void_p, C.c_uint64]
        L.pvol_radiance_gather_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(abi.GatherParams),
                                                 C.POINTER(abi.RadianceGatherOut)]
        L.pvol_radiance_gather_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(abi.GatherParams),
                                                        C.POINTER(abi.RadianceGatherOut), C.c_void_p]
        L.pvol_radiance_gather_check.argtypes = [C.c_int, C.POINTER(abi.RadianceGatherCheck), C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                                 C.c_uint32]
        L.pvol_radiance_gather_slice.argtypes = [C.c_int32, C.c_uint64]
        L.pvol_radiance_gather_slice.restype = C.c_uint32
        L.pvol_probe_hits.argtypes =[C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, _f32p, C.POINTER(C.c_int32)]
        L.pvol_set_surface_integrator.argtypes = [C.c_void_p, C.POINTER(abi.SurfaceParams), _f32p, _f32p, _f32p, C.c_uint32]
        L.pvol_set_surface_integrator_maps.argtypes = [C.c_void_p, C.POINTER(abi.SurfaceParams), C.POINTER(abi.PhotonArray), C.POINTER(abi.PhotonArray)]
        L.pvol_check_surface_maps.argtypes = [C.POINTER(abi.SurfaceParams), C.c_int, C.c_int, C.c_int, _u32p, _u32p, C.POINTER(abi.PhotonArray),
                                              C.POINTER(abi.PhotonArray), C.c_int]
        L.pvol_march_kernel_name.restype = C.c_char_p
        L.pvol_tile_kernel_name.argtypes = [C.c_void_p]
        L.pvol_tile_kernel_name.restype = C.c_char_p
        L.pvol_tile_form_name.argtypes = [C.c_void_p]
        L.pvol_tile_form_name.restype = C.c_char_p
        L.pvol_gaussian_filter_table.argtypes = [C.c_float, C.c_float, C.c_float, _f32p]
        L.pvol_gaussian_filter_table.restype = None
        L.pvol_compute_sub_window.argtypes = [C.POINTER(abi.Sampler), C.c_uint32, C.POINTER(C.c_int32)]
        L.pvol_compute_sub_window.restype = None
        L.pvol_render_sample_count.argtypes = [C.POINTER(abi.Sampler), _u32p, C.c_uint32]
        L.pvol_render_sample_count.restype = C.c_uint64
        L.pvol_render_tasks_device.argtypes = [C.c_void_p, C.POINTER(abi.Camera), C.POINTER(abi.Film), C.POINTER(abi.Sampler), _u32p, C.c_uint32,
                                               C.c_void_p, C.POINTER(abi.RenderDebug), C.c_void_p]
        L.pvol_film_add_samples_device.argtypes = [C.c_void_p, C.POINTER(abi.Film), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        L.pvol_film_resolve_device.argtypes = [C.c_void_p, C.POINTER(abi.Film), C.c_void_p, C.c_void_p, C.c_void_p]
        L.pvol_partition_tasks.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _u32p]
        L.pvol_render_frame_ranks.argtypes = [C.c_void_p, C.POINTER(abi.Camera), C.POINTER(abi.Film), C.POINTER(abi.Sampler), C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pvol_preprocess_group.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32]
        L.pvol_render_frame_group.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(abi.Camera), C.POINTER(abi.Film), C.POINTER(abi.Sampler),
                                              C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p)]
        _cam, _film, _win, _smp = C.POINTER(abi.Camera), C.POINTER(abi.Film), C.POINTER(abi.FilmWindow), C.POINTER(abi.Sampler)
        L.pvol_film_window_from_crop.argtypes = [_film, _f32p, _win]
        L.pvol_film_sample_extent.argtypes = [_film, _win, C.POINTER(C.c_int32)]
        L.pvol_render_tasks_window_device.argtypes = [C.c_void_p, _cam, _film, _win, _smp, _u32p, C.c_uint32, C.c_void_p, C.POINTER(abi.RenderDebug),
                                                      C.c_void_p]
        L.pvol_film_add_samples_window_device.argtypes = [C.c_void_p, _film, _win, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        L.pvol_film_resolve_window_device.argtypes = [C.c_void_p, _film, _win, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pvol_render_frame_ranks_window.argtypes = [C.c_void_p, _cam, _film, _win, _smp, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]
        L.pvol_render_frame_group_window.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, _cam, _film, _win, _smp, C.POINTER(C.c_void_p), C.c_void_p,
                                                     C.POINTER(C.c_void_p)]
        L.pvol_enable_phase_timing.argtypes = [C.c_void_p, C.c_int]
        L.pvol_get_phase_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        _lib = L
    return _lib


EXPORTS = ["pvol_abi_version", "pvol_strerror", "pvol_device_count", "pvol_default_params", "pvol_create",
           "pvol_destroy", "pvol_set_scene", "pvol_upload_photons", "pvol_preprocess", "pvol_photon_count",
           "pvol_download_photons", "pvol_li_batch", "pvol_li_batch_device", "pvol_li", "pvol_transmittance_batch",
           "pvol_get_stats", "pvol_enable_stats", "pvol_kernel_time_ms", "pvol_get_shoot_stats",
           "pvol_gaussian_filter_table", "pvol_compute_sub_window", "pvol_render_sample_count", "pvol_render_tasks_device",
           "pvol_film_add_samples_device", "pvol_film_resolve_device", "pvol_march_kernel_name", "pvol_check_errors", "pvol_get_preprocess_seconds", "pvol_get_accel_info", "pvol_surface_photon_count",
           "pvol_download_surface_photons", "pvol_radiance_photon_count", "pvol_download_radiance_photons",
           "pvol_set_surface_integrator", "pvol_enable_phase_timing", "pvol_get_phase_ms",
           "pvol_partition_tasks", "pvol_render_frame_ranks", "pvol_preprocess_blocks",
           "pvol_preprocess_ranks", "pvol_get_exchange_seconds", "pvol_li_many", "pvol_set_li_coalescing",
           "pvol_get_li_coalescing_stats", "pvol_preprocess_group", "pvol_render_frame_group",
           "pvol_film_window_from_crop", "pvol_film_sample_extent", "pvol_render_tasks_window_device",
           "pvol_film_add_samples_window_device", "pvol_film_resolve_window_device", "pvol_render_frame_ranks_window",
           "pvol_render_frame_group_window", "pvol_tile_kernel_name", "pvol_tile_form_name", "pvol_set_triangle_normals",
           "pvol_compute_radiance", "pvol_compute_radiance_arrays", "pvol_radiance_lo_count", "pvol_download_radiance_lo",
           "pvol_radiance_lookup", "pvol_radiance_lookup_device", "pvol_set_surface_integrator_maps",
           "pvol_build_gather_map", "pvol_build_gather_map_arrays", "pvol_gather_map_count", "pvol_gather_photons",
           "pvol_gather_photons_device", "pvol_gather_directions", "pvol_gather_directions_device", "pvol_final_gather",
           "pvol_final_gather_device", "pvol_lphoton_batch", "pvol_lphoton_batch_device", "pvol_radiance_batch",
           "pvol_radiance_batch_device", "pvol_radiance_gather_batch", "pvol_radiance_gather_batch_device",
           "pvol_set_volume_integrator", "pvol_get_volume_integrator"]

VOLUME_INTEGRATORS = {"photonvolume": abi.VOLINT_PHOTON, "single": abi.VOLINT_SINGLE}   # core/api.cpp:575-581 by name

SHOOT_STAT_NAMES = ["paths", "follow_calls", "no_hit", "march_steps", "interactions", "absorbed", "stored_volume",
                    "stored_caustic", "stored_direct", "stored_indirect", "split_children", "nshot"]


def partition_tasks(n_tasks, rank, n_ranks):
    """pvol_partition_tasks: the task numbers rank `rank` of `n_ranks` renders (pure host code: needs no GPU)."""
    n = C.c_uint32()
    _check(lib().pvol_partition_tasks(n_tasks, rank, n_ranks, None, 0, C.byref(n)), "pvol_partition_tasks")
    ids = np.zeros(n.value, np.uint32)
    _check(lib().pvol_partition_tasks(n_tasks, rank, n_ranks, ids.ctypes.data_as(_u32p), n.value, C.byref(n)), "pvol_partition_tasks")
    return ids


def _ptrs(values):
    """A C array of pointers (integers, 0 / None = NULL)."""
    return (C.c_void_p * len(values))(*[v or None for v in values])


def preprocess_group(pvs, n_tasks, block_paths=4096):
    """pvol_preprocess_group: preprocess(n_tasks, block_paths) sharded over the contexts `pvs` (a list of PhotonVolume, one host
    thread each, joined by an in-process all-gather); every context ends with the single-context map, bit for bit."""
    _check(lib().pvol_preprocess_group(_ptrs([pv._h.value for pv in pvs]), len(pvs), n_tasks, block_paths), "pvol_preprocess_group")


def render_frame_group(pvs, cam, film, smp, d_pixels, d_rgb, hip_streams=None, window=None):
    """pvol_render_frame_group: one frame over the contexts `pvs`.  d_pixels: one full-frame film per context (device pointers, on
    that context's device), d_rgb on the first context's device (0: no resolve), hip_streams: one per context (None: null streams).
    Enqueued on hip_streams[0]: synchronise it (or the first context's device) before reading d_pixels[0] / d_rgb.
    window (an abi.FilmWindow): pvol_render_frame_group_window, every film, the sum and d_rgb hold the window's pixels."""
    if len(d_pixels) != len(pvs) or (hip_streams is not None and len(hip_streams) != len(pvs)):
        raise ValueError("render_frame_group: one film (and stream) per context")
    streams = None if hip_streams is None else _ptrs(list(hip_streams))
    if window is not None:
        _check(lib().pvol_render_frame_group_window(_ptrs([pv._h.value for pv in pvs]), len(pvs), C.byref(cam), C.byref(film), C.byref(window),
                                                    C.byref(smp), _ptrs(list(d_pixels)), d_rgb or None, streams), "pvol_render_frame_group_window")
        return
    _check(lib().pvol_render_frame_group(_ptrs([pv._h.value for pv in pvs]), len(pvs), C.byref(cam), C.byref(film), C.byref(smp),
                                         _ptrs(list(d_pixels)), d_rgb or None, streams), "pvol_render_frame_group")


def _check(rc, where):
    if rc != abi.PVOL_OK:
        raise PvolError(rc, where)


def photon_array(m):
    """One map (p[n,3], wi[n,3], alpha[n,30], n_paths) as (a pvol_photon_array, what keeps its arrays alive); None stays None."""
    if m is None:
        return None, None
    p, w, a = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in m[:3])
    n = p.size // 3
    if w.size != 3 * n or a.size != 30 * n:
        raise ValueError("photon arrays disagree: %d positions, %d directions, %d weights" % (n, w.size // 3, a.size // 30))
    return abi.PhotonArray(p.ctypes.data_as(_f32p), w.ctypes.data_as(_f32p), a.ctypes.data_as(_f32p), n, int(m[3])), (p, w, a)


def photon_arrays(maps):
    """maps: three entries in the `kind` order (caustic, direct, indirect), each None or (p[n,3], wi[n,3], alpha[n,30], n_paths).
    Returns (the pvol_photon_array *[3] for pvol_compute_radiance_arrays, what keeps its arrays alive)."""
    if len(maps) != 3:
        raise ValueError("three maps (caustic, direct, indirect), got %d" % len(maps))
    ptrs = (C.POINTER(abi.PhotonArray) * 3)()
    keep = []
    for i, m in enumerate(maps):
        if m is None:
            continue
        p, w, a = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in m[:3])
        n = p.size // 3
        if w.size != 3 * n or a.size != 30 * n:
            raise ValueError("photon arrays disagree: %d positions, %d directions, %d weights" % (n, w.size // 3, a.size // 30))
        pa = abi.PhotonArray(p.ctypes.data_as(_f32p), w.ctypes.data_as(_f32p), a.ctypes.data_as(_f32p), n, int(m[3]))
        keep.append((pa, p, w, a))
        ptrs[i] = C.pointer(pa)
    return ptrs, keep


class PhotonVolume:
    """Host-side mirror of the reference's plugin surface for this path: construct from the
    integrator/shooter parameters (CreatePhotonVolumeIntegrator / CreatePhotonShooter), hand it the
    scene, `preprocess()` or `upload_photons()`, then `li()` / `transmittance()`."""

    def __init__(self, params):
        self._h = C.c_void_p()
        self.params = params
        _check(lib().pvol_create(C.byref(params), C.byref(self._h)), "pvol_create")
        self._scene = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().pvol_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, holder):
        self._scene = holder  # keeps the ctypes arrays alive
        _check(lib().pvol_set_scene(self._h, C.byref(holder.scene)), "pvol_set_scene")
        if getattr(holder, "tri_normals", None) is not None:
            self.set_triangle_normals(holder.tri_normals)

    def set_triangle_normals(self, n):
        """pvol_set_triangle_normals: n[n_triangles, 9], the world-space vertex normals of every triangle of the scene set last (nine
        zeros: none for that triangle); None clears them.  set_scene() does this itself for a holder whose dictionary has "tris.n"."""
        if n is None:
            _check(lib().pvol_set_triangle_normals(self._h, None, 0), "pvol_set_triangle_normals")
            return
        n = np.ascontiguousarray(n, np.float32).reshape(-1, 9)
        _check(lib().pvol_set_triangle_normals(self._h, n.ctypes.data_as(_f32p), len(n)), "pvol_set_triangle_normals")

    def upload_photons(self, p, wi, alpha):
        p = np.ascontiguousarray(p, np.float32).reshape(-1)
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1)
        alpha = np.ascontiguousarray(alpha, np.float32).reshape(-1)
        n = p.size // 3
        if wi.size != 3 * n or alpha.size != 30 * n:
            raise ValueError("photon arrays disagree: %d positions, %d directions, %d weights" % (n, wi.size // 3, alpha.size // 30))
        _check(lib().pvol_upload_photons(self._h, p.ctypes.data_as(_f32p), wi.ctypes.data_as(_f32p), alpha.ctypes.data_as(_f32p), n),
               "pvol_upload_photons")

    def preprocess(self, n_tasks=1, block_paths=4096):
        """PhotonShooter::Preprocess on the device; block_paths < 4096: many small blocks (pvol_preprocess_blocks)."""
        if block_paths == 4096:
            _check(lib().pvol_preprocess(self._h, n_tasks), "pvol_preprocess")
        else:
            _check(lib().pvol_preprocess_blocks(self._h, n_tasks, block_paths), "pvol_preprocess_blocks")

    def preprocess_ranks(self, n_tasks, rank, n_ranks, *, allgather=None, nccl_comm=None, block_paths=4096):
        """This rank's share of preprocess(n_tasks, block_paths) sharded over n_ranks ranks (pvol_preprocess_ranks): every rank
        ends with the single-rank map, bit for bit.  Exactly one transport: `allgather`, a callable bytes -> list of n_ranks bytes
        (e.g. gloo_allgather()), or `nccl_comm`, an ncclComm_t (integer) of n_ranks ranks."""
        comm = ShootComm()
        err = []
        cb = None
        if allgather is not None:
            def _cb(user, send, recv, nbytes):
                try:
                    parts = allgather(C.string_at(send, nbytes) if nbytes else b"")
                    if len(parts) != n_ranks or any(len(p) != nbytes for p in parts):
                        raise ValueError("allgather returned %d parts of %s bytes, wanted %d of %d"
                                         % (len(parts), sorted({len(p) for p in parts}), n_ranks, nbytes))
                    if nbytes:
                        C.memmove(recv, b"".join(parts), nbytes * n_ranks)
                    return 0
                except BaseException as e:   # noqa: B902 -- must not unwind through C; re-raised below
                    err.append(e)
                    return 1
            cb = ALLGATHER_FN(_cb)   # kept alive by this frame for the whole call
            comm.allgather = cb
        if nccl_comm is not None:
            comm.nccl_comm = nccl_comm
        rc = lib().pvol_preprocess_ranks(self._h, n_tasks, block_paths, rank, n_ranks, C.byref(comm))
        del cb
        if err:
            raise PvolError(rc, "pvol_preprocess_ranks") from err[0]
        _check(rc, "pvol_preprocess_ranks")

    def exchange_seconds(self):
        """Seconds the last preprocess_ranks() spent in its all-gathers (part of preprocess_times()[0])."""
        v = C.c_double()
        _check(lib().pvol_get_exchange_seconds(self._h, C.byref(v)), "pvol_get_exchange_seconds")
        return float(v.value)

    def preprocess_times(self):
        """(shoot seconds, search-structure build seconds) of the last preprocess()."""
        v = (C.c_double * 2)()
        _check(lib().pvol_get_preprocess_seconds(self._h, v), "pvol_get_preprocess_seconds")
        return float(v[0]), float(v[1])

    def accel_info(self):
        """(triangles in the device-built hierarchy -- 0 when the scene is scanned linearly --, build milliseconds)."""
        v = (C.c_double * 2)()
        _check(lib().pvol_get_accel_info(self._h, v), "pvol_get_accel_info")
        return int(v[0]), float(v[1])

    def probe_hits(self, rays, mode):
        """The tests' ray probe (csrc/pvol_probe.hip, not part of the ABI): rays (RAY_DTYPE) through the device's own hit routines on
        the uploaded scene -- mode 0 surf_closest, 1 lane_occluded, 2 scene_occluded (one ray per wave), 3 scene_closest (the photon
        shooter's closest hit, one ray per wave, maxt = inf; the record of mode 0).  Returns (f, i): f[n, 11] = t, rayEps, p, nn, dpdu; i[n, 3] = hit flag, primitive (triangle index in upload order, -1 - k for sphere k), material."""
        assert rays.dtype == abi.RAY_DTYPE
        rays = np.ascontiguousarray(rays)
        f = np.zeros((len(rays), 11), np.float32)
        i = np.zeros((len(rays), 3), np.int32)
        _check(lib().pvol_probe_hits(self._h, rays.ctypes.data, len(rays), mode, f.ctypes.data_as(_f32p), i.ctypes.data_as(C.POINTER(C.c_int32))),
               "pvol_probe_hits")
        return f, i

    def surface_photons(self, kind):
        """(p, wo, alpha, n_paths) of the caustic (0) / direct (1) / indirect (2) store kept by the last preprocess()."""
        n, npaths = C.c_uint32(), C.c_uint32()
        _check(lib().pvol_surface_photon_count(self._h, kind, C.byref(n), C.byref(npaths)), "pvol_surface_photon_count")
        p, wo, a = np.zeros((n.value, 3), np.float32), np.zeros((n.value, 3), np.float32), np.zeros((n.value, 30), np.float32)
        _check(lib().pvol_download_surface_photons(self._h, kind, p.ctypes.data_as(_f32p), wo.ctypes.data_as(_f32p), a.ctypes.data_as(_f32p), n.value),
               "pvol_download_surface_photons")
        return p, wo, a, int(npaths.value)

    def radiance_photons(self):
        """(p, n, rho_r, rho_t) of the radiance photons kept by the last preprocess()."""
        n = C.c_uint32()
        _check(lib().pvol_radiance_photon_count(self._h, C.byref(n)), "pvol_radiance_photon_count")
        p, nn = np.zeros((n.value, 3), np.float32), np.zeros((n.value, 3), np.float32)
        rr, rt = np.zeros((n.value, 30), np.float32), np.zeros((n.value, 30), np.float32)
        _check(lib().pvol_download_radiance_photons(self._h, p.ctypes.data_as(_f32p), nn.ctypes.data_as(_f32p), rr.ctypes.data_as(_f32p),
                                                    rt.ctypes.data_as(_f32p), n.value), "pvol_download_radiance_photons")
        return p, nn, rr, rt

    def compute_radiance(self, n_lookup, max_dist, maps=None, radiance=None):
        """ComputeRadianceTask on the device (photonshooter.cpp:359-395).  Without arguments: over the stores the last preprocess()
        kept (pvol_compute_radiance).  Otherwise maps = [caustic, direct, indirect], each None or (p, wi, alpha, n_paths), and
        radiance = (p[n,3], n[n,3], rho_r[n,30], rho_t[n,30]) (pvol_compute_radiance_arrays)."""
        if maps is None and radiance is None:
            _check(lib().pvol_compute_radiance(self._h, int(n_lookup), float(max_dist)), "pvol_compute_radiance")
            return
        if maps is None or radiance is None:
            raise ValueError("compute_radiance: maps and radiance go together")
        ptrs, keep = photon_arrays(maps)
        p, nn, rr, rt = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in radiance)
        n = p.size // 3
        if nn.size != 3 * n or rr.size != 30 * n or rt.size != 30 * n:
            raise ValueError("radiance photon arrays disagree on their count")
        _check(lib().pvol_compute_radiance_arrays(self._h, int(n_lookup), float(max_dist), ptrs, p.ctypes.data_as(_f32p), nn.ctypes.data_as(_f32p),
                                                  rr.ctypes.data_as(_f32p), rt.ctypes.data_as(_f32p), n), "pvol_compute_radiance_arrays")
        del keep

    def radiance_lo_count(self):
        n = C.c_uint32()
        _check(lib().pvol_radiance_lo_count(self._h, C.byref(n)), "pvol_radiance_lo_count")
        return n.value

    def radiance_lo(self):
        """(p[n,3], n[n,3], lo[n,30]) of the last compute_radiance(), in input order."""
        n = self.radiance_lo_count()
        p, nn, lo = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 30), np.float32)
        _check(lib().pvol_download_radiance_lo(self._h, p.ctypes.data_as(_f32p), nn.ctypes.data_as(_f32p), lo.ctypes.data_as(_f32p), n),
               "pvol_download_radiance_lo")
        return p, nn, lo

    def radiance_lookup(self, p, n):
        """The radiance map's nearest photon facing n at every point p (RadiancePhotonProcess): (lo[count,30], found[count])."""
        p = np.ascontiguousarray(p, np.float32).reshape(-1)
        n = np.ascontiguousarray(n, np.float32).reshape(-1)
        count = p.size // 3
        if n.size != 3 * count:
            raise ValueError("radiance_lookup: %d points, %d normals" % (count, n.size // 3))
        lo, found = np.zeros((count, 30), np.float32), np.zeros(count, np.uint32)
        _check(lib().pvol_radiance_lookup(self._h, p.ctypes.data_as(_f32p), n.ctypes.data_as(_f32p), count, lo.ctypes.data_as(_f32p),
                                          found.ctypes.data_as(_u32p)), "pvol_radiance_lookup")
        return lo, found

    def radiance_lookup_device(self, d_p, d_n, count, d_lo, d_found, hip_stream=0):
        """Device-pointer variant (integers): enqueue only, no synchronisation."""
        _check(lib().pvol_radiance_lookup_device(self._h, d_p, d_n, count, d_lo, d_found, hip_stream), "pvol_radiance_lookup_device")

    def build_gather_map(self, indirect=None):
        """The gather map (the indirect map as the reference's kd-tree): from the indirect store the last preprocess() kept
        (pvol_build_gather_map), or from indirect = (p[n,3], wi[n,3]) (pvol_build_gather_map_arrays).  Returns its photon count."""
        if indirect is None:
            _check(lib().pvol_build_gather_map(self._h), "pvol_build_gather_map")
        else:
            p, w = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in indirect[:2])
            if w.size != p.size:
                raise ValueError("build_gather_map: %d positions, %d directions" % (p.size // 3, w.size // 3))
            pa = abi.PhotonArray(p.ctypes.data_as(_f32p), w.ctypes.data_as(_f32p), None, p.size // 3, 0)
            _check(lib().pvol_build_gather_map_arrays(self._h, C.byref(pa)), "pvol_build_gather_map_arrays")
        return self.gather_map_count()

    def gather_map_count(self):
        n = C.c_uint32()
        _check(lib().pvol_gather_map_count(self._h, C.byref(n)), "pvol_gather_map_count")
        return n.value

    def gather_photons(self, p, max_dist):
        """The 50 indirect photons of the final gather at every point p, in the order of PhotonProcess' heap
        (photonmap.cpp:189-199): (index[count,50] in the store's order, d2[count,50], found[count], rounds[count])."""
        p = np.ascontiguousarray(p, np.float32).reshape(-1)
        count = p.size // 3
        index, d2 = np.zeros((count, GATHER_K), np.uint32), np.zeros((count, GATHER_K), np.float32)
        found, rounds = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
        _check(lib().pvol_gather_photons(self._h, p.ctypes.data_as(_f32p), count, float(max_dist), index.ctypes.data_as(_u32p),
                                         d2.ctypes.data_as(_f32p), found.ctypes.data_as(_u32p), rounds.ctypes.data_as(_u32p)), "pvol_gather_photons")
        return index, d2, found, rounds

    def gather_photons_device(self, d_p, count, max_dist, d_index, d_d2, d_found, d_rounds, hip_stream=0):
        """Device-pointer variant (integers): enqueue only, no synchronisation."""
        _check(lib().pvol_gather_photons_device(self._h, d_p, count, float(max_dist), d_index, d_d2, d_found, d_rounds, hip_stream),
               "pvol_gather_photons_device")

    def gather_directions(self, p, frames, wo, max_dist, cos_gather_angle, u_bsdf, u_photon):
        """The gather rays of both sampling loops (photonmap.cpp:208-219, :250-265) with their weights.  frames[count,9] = nn, dpdu,
        ng; wo[count,3]; u_bsdf, u_photon[count,n_samples,3] = uComponent, uDir[0], uDir[1].  Returns two GATHER_SAMPLE_DTYPE
        arrays [count, n_samples]: the BSDF-sampled and the photon-sampled rays."""
        p, frames, wo = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in (p, frames, wo))
        u_bsdf, u_photon = np.ascontiguousarray(u_bsdf, np.float32), np.ascontiguousarray(u_photon, np.float32)
        count = p.size // 3
        if u_bsdf.ndim != 3 or u_bsdf.shape != u_photon.shape or u_bsdf.shape[0] != count or u_bsdf.shape[2] != 3:
            raise ValueError("gather_directions: u_bsdf and u_photon are [count, n_samples, 3]")
        if frames.size != 9 * count or wo.size != 3 * count:
            raise ValueError("gather_directions: %d points, %d frames, %d wo" % (count, frames.size // 9, wo.size // 3))
        ns = u_bsdf.shape[1]
        ob, op = np.zeros((count, ns), GATHER_SAMPLE_DTYPE), np.zeros((count, ns), GATHER_SAMPLE_DTYPE)
        _check(lib().pvol_gather_directions(self._h, p.ctypes.data_as(_f32p), frames.ctypes.data_as(_f32p), wo.ctypes.data_as(_f32p), count,
                                            float(max_dist), ns, float(cos_gather_angle), u_bsdf.ctypes.data_as(_f32p), u_photon.ctypes.data_as(_f32p),
                                            ob.ctypes.data, op.ctypes.data), "pvol_gather_directions")
        return ob, op

    def gather_directions_device(self, d_p, d_frames, d_wo, count, max_dist, n_samples, cos_gather_angle, d_u_bsdf, d_u_photon, d_out_bsdf,
                                 d_out_photon, hip_stream=0):
        """Device-pointer variant (integers): enqueue only, no synchronisation."""
        _check(lib().pvol_gather_directions_device(self._h, d_p, d_frames, d_wo, count, float(max_dist), int(n_samples), float(cos_gather_angle),
                                                   d_u_bsdf, d_u_photon, d_out_bsdf, d_out_photon, hip_stream), "pvol_gather_directions_device")

    def final_gather(self, p, frames, wo, kd, ray_eps, max_dist, cos_gather_angle, u_bsdf, u_photon, rays=False):
        """The final gather at every point p (photonmap.cpp:183-295 for a Lambertian hit): the gather rays of gather_directions()
        traced, Lindir from the radiance map, the homogeneous medium's transmittance, and both loops' weighted sums.  kd[count,30],
        ray_eps[count]; n_samples is u_bsdf.shape[1].  Returns (L[count,30], draws[count]) and, with rays=True, a third item
        (rays_bsdf, rays_photon): two GATHER_RAY_DTYPE arrays [count, n_samples]."""
        p, frames, wo, kd, ray_eps = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in (p, frames, wo, kd, ray_eps))
        u_bsdf, u_photon = np.ascontiguousarray(u_bsdf, np.float32), np.ascontiguousarray(u_photon, np.float32)
        count = p.size // 3
        if u_bsdf.ndim != 3 or u_bsdf.shape != u_photon.shape or u_bsdf.shape[0] != count or u_bsdf.shape[2] != 3:
            raise ValueError("final_gather: u_bsdf and u_photon are [count, n_samples, 3]")
        if frames.size != 9 * count or wo.size != 3 * count or kd.size != 30 * count or ray_eps.size != count:
            raise ValueError("final_gather: %d points, %d frames, %d wo, %d kd, %d ray_eps" % (count, frames.size // 9, wo.size // 3, kd.size // 30,
                                                                                             ray_eps.size))
        ns = u_bsdf.shape[1]
        L, draws = np.zeros((count, 30), np.float32), np.zeros(count, np.uint32)
        rb = np.zeros((count, ns), GATHER_RAY_DTYPE) if rays else None
        rp = np.zeros((count, ns), GATHER_RAY_DTYPE) if rays else None
        _check(lib().pvol_final_gather(self._h, p.ctypes.data_as(_f32p), frames.ctypes.data_as(_f32p), wo.ctypes.data_as(_f32p),
                                       kd.ctypes.data_as(_f32p), ray_eps.ctypes.data_as(_f32p), count, float(max_dist), ns, float(cos_gather_angle),
                                       u_bsdf.ctypes.data_as(_f32p), u_photon.ctypes.data_as(_f32p), L.ctypes.data_as(_f32p),
                                       draws.ctypes.data_as(_u32p), rb.ctypes.data if rays else None, rp.ctypes.data if rays else None),
               "pvol_final_gather")
        return (L, draws, (rb, rp)) if rays else (L, draws)

    def final_gather_device(self, d_p, d_frames, d_wo, d_kd, d_ray_eps, count, max_dist, n_samples, cos_gather_angle, d_u_bsdf, d_u_photon, d_L,
                            d_draws, d_rays_bsdf=0, d_rays_photon=0, hip_stream=0):
        """Device-pointer variant (integers): enqueue only, no synchronisation."""
        _check(lib().pvol_final_gather_device(self._h, d_p, d_frames, d_wo, d_kd, d_ray_eps, count, float(max_dist), int(n_samples),
                                              float(cos_gather_angle), d_u_bsdf, d_u_photon, d_L, d_draws, d_rays_bsdf or None,
                                              d_rays_photon or None, hip_stream), "pvol_final_gather_device")

    def final_gather_set_scratch_bound(self, nbytes):
        """Test hook: the bytes of scratch a slice of final_gather() may take (0: the header's PVOL_FINAL_GATHER_SCRATCH_BYTES)."""
        _check(lib().pvol_final_gather_set_scratch_bound(self._h, int(nbytes)), "pvol_final_gather_set_scratch_bound")

    def lphoton_batch(self, points, w=None, output_kind=abi.OUT_SPECTRAL, want_counts=False):
        """LPhoton (photonvolume.cpp:65-108) on the current volume map at points[n,3], in the caller's order: L[n,30], or X, Y, Z, 0
        with OUT_XYZ.  w[n,3]: the direction LPhoton is given; None only where the medium's g is 0.  want_counts: also
        (n_found[n], radius2[n]) -- proc.nFound and the largest kept fp32 distance^2."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1)
        n = p.size // 3
        if w is not None:
            w = np.ascontiguousarray(w, np.float32).reshape(-1)
            if w.size != 3 * n:
                raise ValueError("lphoton_batch: %d points, %d directions" % (n, w.size // 3))
        out = np.zeros((n, 30 if output_kind == abi.OUT_SPECTRAL else 4), np.float32)
        found, r2 = (np.zeros(n, np.uint32), np.zeros(n, np.float32)) if want_counts else (None, None)
        _check(lib().pvol_lphoton_batch(self._h, p.ctypes.data_as(_f32p), w.ctypes.data_as(_f32p) if w is not None else None, n, int(output_kind),
                                        out.ctypes.data_as(_f32p), found.ctypes.data_as(_u32p) if want_counts else None,
                                        r2.ctypes.data_as(_f32p) if want_counts else None), "pvol_lphoton_batch")
        return (out, found, r2) if want_counts else out

    def lphoton_batch_device(self, d_p, d_w, n, output_kind, d_out, d_n_found=0, d_radius2=0, hip_stream=0):
        """Device-pointer variant (integers; d_w, d_n_found, d_radius2 may be 0): enqueue only, no synchronisation."""
        _check(lib().pvol_lphoton_batch_device(self._h, d_p, d_w or None, n, int(output_kind), d_out, d_n_found or None, d_radius2 or None, hip_stream),
               "pvol_lphoton_batch_device")

    def lphoton_set_scratch_bound(self, nbytes):
        """Test hook: the bytes of ordering scratch a slice of lphoton_batch() may take (0: the header's PVOL_LPHOTON_SCRATCH_BYTES)."""
        _check(lib().pvol_lphoton_set_scratch_bound(self._h, int(nbytes)), "pvol_lphoton_set_scratch_bound")

    def radiance_batch(self, rays, streams, output_kind=abi.OUT_SPECTRAL, want=()):
        """SamplerRenderer::Li for the caller's own rays (pvol_radiance_batch): Scene::Intersect clips each ray, the surface integrator
        (if one is on) runs at the hit, specular recursion included, then the volume Li().  Returns a dict: "L"[n, 60|4] = T * Ls + Lvi
        then T, and the optional outputs named in `want` (abi.RADIANCE_WANT): "surf_xyz"[n,3], "t_hit"[n], "draws"[n], "surf_draws"[n],
        "n_segments"[n].  rays['rng_skip'] holds the caller's own draws only; streams['end_draw'] is updated."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype == abi.RAY_DTYPE and streams.dtype == abi.STREAM_DTYPE and streams.flags["C_CONTIGUOUS"]
        n = len(rays)
        res = {"L": np.zeros((n, 60 if output_kind == abi.OUT_SPECTRAL else 4), np.float32)}
        for k in want:
            if k not in abi.RADIANCE_WANT:
                raise ValueError("radiance_batch: unknown output %r" % (k,))
            res[k] = np.zeros((n, 3), np.float32) if k == "surf_xyz" else np.zeros(n, np.float32 if k == "t_hit" else np.uint32)
        out = abi.RadianceOut(**{k: v.ctypes.data for k, v in res.items()})
        _check(lib().pvol_radiance_batch(self._h, rays.ctypes.data, n, streams.ctypes.data, len(streams), int(output_kind), C.byref(out)),
               "pvol_radiance_batch")
        return res

    def radiance_batch_device(self, d_rays, n_rays, d_streams, n_streams, output_kind, d_L, hip_stream=0, **d_optional):
        """Device-pointer variant (integers; d_optional: surf_xyz=, t_hit=, draws=, surf_draws=, n_segments=).  Enqueued on hip_stream,
        which is synchronised once for the stream table and once per slice; the last slice's kernels are left in flight."""
        for k in d_optional:
            if k not in abi.RADIANCE_WANT:
                raise ValueError("radiance_batch_device: unknown output %r" % (k,))
        out = abi.RadianceOut(L=d_L or None, **{k: (v or None) for k, v in d_optional.items()})
        _check(lib().pvol_radiance_batch_device(self._h, d_rays, n_rays, d_streams, n_streams, int(output_kind), C.byref(out), hip_stream),
               "pvol_radiance_batch_device")

    def radiance_gather_batch(self, rays, streams, max_dist, cos_gather_angle, u_bsdf, u_photon, output_kind=abi.OUT_SPECTRAL, want=()):
        """radiance_batch() with the final gather (photonmap.cpp:183-296) at every Lambertian hit of every ray and spawned ray
        (pvol_radiance_gather_batch).  u_bsdf, u_photon: [n, n_samples, 3] per CALLER ray, shared by the rays it spawns; max_dist,
        cos_gather_angle as for final_gather().  Needs a gather map, a radiance result and a surface integrator without an indirect
        map.  `want` may also name "gather_draws"[n] (abi.RADIANCE_GATHER_WANT)."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype == abi.RAY_DTYPE and streams.dtype == abi.STREAM_DTYPE and streams.flags["C_CONTIGUOUS"]
        n = len(rays)
        u_bsdf, u_photon = np.ascontiguousarray(u_bsdf, np.float32), np.ascontiguousarray(u_photon, np.float32)
        if u_bsdf.ndim != 3 or u_bsdf.shape != u_photon.shape or u_bsdf.shape[0] != n or u_bsdf.shape[2] != 3:
            raise ValueError("radiance_gather_batch: u_bsdf and u_photon are [n_rays, n_samples, 3]")
        res = {"L": np.zeros((n, 60 if output_kind == abi.OUT_SPECTRAL else 4), np.float32)}
        for k in want:
            if k not in abi.RADIANCE_GATHER_WANT:
                raise ValueError("radiance_gather_batch: unknown output %r" % (k,))
            res[k] = np.zeros((n, 3), np.float32) if k == "surf_xyz" else np.zeros(n, np.float32 if k == "t_hit" else np.uint32)
        out = abi.RadianceGatherOut(**{k: v.ctypes.data for k, v in res.items()})
        g = abi.GatherParams(float(max_dist), int(u_bsdf.shape[1]), float(cos_gather_angle), u_bsdf.ctypes.data, u_photon.ctypes.data)
        _check(lib().pvol_radiance_gather_batch(self._h, rays.ctypes.data, n, streams.ctypes.data, len(streams), int(output_kind), C.byref(g),
                                                C.byref(out)), "pvol_radiance_gather_batch")
        return res

    def radiance_gather_batch_device(self, d_rays, n_rays, d_streams, n_streams, max_dist, n_samples, cos_gather_angle, d_u_bsdf, d_u_photon,
                                     output_kind, d_L, hip_stream=0, **d_optional):
        """Device-pointer variant (integers; d_optional: radiance_batch_device's and gather_draws=); synchronises hip_stream as
        radiance_batch_device does."""
        for k in d_optional:
            if k not in abi.RADIANCE_GATHER_WANT:
                raise ValueError("radiance_gather_batch_device: unknown output %r" % (k,))
        out = abi.RadianceGatherOut(L=d_L or None, **{k: (v or None) for k, v in d_optional.items()})
        g = abi.GatherParams(float(max_dist), int(n_samples), float(cos_gather_angle), d_u_bsdf or None, d_u_photon or None)
        _check(lib().pvol_radiance_gather_batch_device(self._h, d_rays, n_rays, d_streams, n_streams, int(output_kind), C.byref(g), C.byref(out),
                                                       hip_stream), "pvol_radiance_gather_batch_device")

    def radiance_set_scratch_bound(self, nbytes):
        """Test hook: the bytes of scratch a slice of radiance_batch() may take (0: the header's PVOL_RADIANCE_SCRATCH_BYTES)."""
        _check(lib().pvol_radiance_set_scratch_bound(self._h, int(nbytes)), "pvol_radiance_set_scratch_bound")

    def check_errors(self):
        """Raises PvolError(PVOL_E_LIMIT) if a batch enqueued through a device entry point hit a kernel limit."""
        _check(lib().pvol_check_errors(self._h), "pvol_check_errors")

    def render_frame_ranks(self, cam, film, smp, rank, n_ranks, nccl_comm, d_pixels, d_rgb=0, hip_stream=0, window=None):
        """One rank of an N-GPU frame behind the C ABI: partition, render, ncclReduce of the film, resolve on rank 0.
        window (an abi.FilmWindow): pvol_render_frame_ranks_window, the films hold the window's pixels."""
        if window is not None:
            _check(lib().pvol_render_frame_ranks_window(self._h, C.byref(cam), C.byref(film), C.byref(window), C.byref(smp), rank, n_ranks, nccl_comm,
                                                        d_pixels, d_rgb, hip_stream), "pvol_render_frame_ranks_window")
            return
        _check(lib().pvol_render_frame_ranks(self._h, C.byref(cam), C.byref(film), C.byref(smp), rank, n_ranks, nccl_comm, d_pixels, d_rgb, hip_stream),
               "pvol_render_frame_ranks")

    def enable_phase_timing(self, on=True):
        _check(lib().pvol_enable_phase_timing(self._h, int(bool(on))), "pvol_enable_phase_timing")

    def phase_ms(self, reset=False):
        """Device milliseconds per phase of render_tasks since the last reset: tile pre-pass, march + gather, surface, film."""
        v = (C.c_double * 6)()
        _check(lib().pvol_get_phase_ms(self._h, v, int(bool(reset))), "pvol_get_phase_ms")
        return {"tile_prepass": v[0], "march_gather": v[2], "surface": v[3], "film_add": v[4]}

    def shoot_stats(self):
        v = (C.c_uint64 * 12)()
        _check(lib().pvol_get_shoot_stats(self._h, v), "pvol_get_shoot_stats")
        return dict(zip(SHOOT_STAT_NAMES, [int(x) for x in v]))

    def photon_count(self):
        n = C.c_uint32()
        _check(lib().pvol_photon_count(self._h, C.byref(n)), "pvol_photon_count")
        return n.value

    def download_photons(self):
        n = self.photon_count()
        p = np.zeros((n, 3), np.float32)
        wi = np.zeros((n, 3), np.float32)
        alpha = np.zeros((n, 30), np.float32)
        _check(lib().pvol_download_photons(self._h, p.ctypes.data_as(_f32p), wi.ctypes.data_as(_f32p), alpha.ctypes.data_as(_f32p), n),
               "pvol_download_photons")
        return p, wi, alpha

    def set_volume_integrator(self, name):
        """pvol_set_volume_integrator: "photonvolume" (the default) or "single" (SingleScatteringIntegrator::Li: no photon map)."""
        if name not in VOLUME_INTEGRATORS:
            raise ValueError('volume integrator %r: "photonvolume" or "single"' % (name,))
        _check(lib().pvol_set_volume_integrator(self._h, VOLUME_INTEGRATORS[name]), "pvol_set_volume_integrator")

    def volume_integrator(self):
        kind = C.c_int()
        _check(lib().pvol_get_volume_integrator(self._h, C.byref(kind)), "pvol_get_volume_integrator")
        return {v: k for k, v in VOLUME_INTEGRATORS.items()}[kind.value]

    def li(self, rays, streams, output_kind=abi.OUT_SPECTRAL):
        """The context's VolumeIntegrator::Li (PhotonVolumeIntegrator unless set_volume_integrator chose another) for a batch; returns (out[n, 60|4], draws[n]); streams['end_draw'] is updated."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype == abi.RAY_DTYPE and streams.dtype == abi.STREAM_DTYPE and streams.flags["C_CONTIGUOUS"]
        n = len(rays)
        out = np.zeros((n, 60 if output_kind == abi.OUT_SPECTRAL else 4), np.float32)
        draws = np.zeros(n, np.uint32)
        _check(lib().pvol_li_batch(self._h, rays.ctypes.data, n, streams.ctypes.data, len(streams), output_kind,
                                   out.ctypes.data_as(_f32p), draws.ctypes.data_as(_u32p)), "pvol_li_batch")
        return out, draws

    def li_device(self, d_rays, n_rays, d_streams, n_streams, output_kind, d_out, d_draws=0, hip_stream=0):
        """Device-pointer variant (integers): enqueue only, no synchronisation."""
        _check(lib().pvol_li_batch_device(self._h, d_rays, n_rays, d_streams, n_streams, output_kind, d_out, d_draws, hip_stream),
               "pvol_li_batch_device")

    # ---- tile driver (device pointers are integers, e.g. torch.Tensor.data_ptr())
    def render_tasks(self, camera, film, sampler, task_ids, d_pixels, debug=None, hip_stream=0, window=None):
        """window (an abi.FilmWindow): pvol_render_tasks_window_device, d_pixels holds the window's pixels and `sampler` its sample
        extent (film_sample_extent)."""
        ids = np.ascontiguousarray(task_ids, np.uint32)
        if window is not None:
            _check(lib().pvol_render_tasks_window_device(self._h, C.byref(camera), C.byref(film), C.byref(window), C.byref(sampler),
                                                         ids.ctypes.data_as(_u32p), len(ids), d_pixels, C.byref(debug) if debug is not None else None,
                                                         hip_stream), "pvol_render_tasks_window_device")
            return
        _check(lib().pvol_render_tasks_device(self._h, C.byref(camera), C.byref(film), C.byref(sampler), ids.ctypes.data_as(_u32p), len(ids),
                                              d_pixels, C.byref(debug) if debug is not None else None, hip_stream), "pvol_render_tasks_device")

    def set_surface_integrator(self, n_used=50, max_dist=0.1, max_specular_depth=5, final_gather=False, caustic=None, n_paths=0,
                               from_preprocess=False, off=False, n_indirect=0):
        """PhotonIntegrator in front of the volume term (CreatePhotonMapSurfaceIntegrator, photonmap.cpp:336-363: nused 50,
        maxdist .1, maxspeculardepth 5).  `caustic` = (p[n,3], wo[n,3], alpha[n,30]) with `n_paths`, or from_preprocess=True to
        take the caustic photons the last preprocess() kept; off=True disables.  Any medium but a VolumeGrid (for which
        render_tasks raises PVOL_E_UNSUPPORTED): none, homogeneous or rainbow, at any nused and phase function, with or without
        a volume photon map, dense enough for the Russian roulette included."""
        if off:
            _check(lib().pvol_set_surface_integrator(self._h, None, None, None, None, 0), "pvol_set_surface_integrator")
            return
        sp = abi.SurfaceParams()
        sp.n_used, sp.max_dist, sp.max_specular_depth, sp.final_gather = int(n_used), float(max_dist), int(max_specular_depth), int(bool(final_gather))
        sp.n_caustic_paths, sp.use_preprocess_store = int(n_paths), int(bool(from_preprocess))
        sp.n_indirect_photons = int(n_indirect)   # the integrator's indirect map, if it has one: refused (PVOL_E_UNSUPPORTED)
        if caustic is None or from_preprocess:
            _check(lib().pvol_set_surface_integrator(self._h, C.byref(sp), None, None, None, 0), "pvol_set_surface_integrator")
            return
        p, w, a = (np.ascontiguousarray(x, np.float32) for x in caustic)
        n = p.size // 3
        assert w.size == 3 * n and a.size == 30 * n
        _check(lib().pvol_set_surface_integrator(self._h, C.byref(sp), p.ctypes.data_as(_f32p), w.ctypes.data_as(_f32p), a.ctypes.data_as(_f32p), n),
               "pvol_set_surface_integrator")

    def set_surface_integrator_maps(self, n_used=50, max_dist=0.1, max_specular_depth=5, final_gather=False, caustic=None, indirect=None,
                                    from_preprocess=False):
        """PhotonIntegrator with both maps of its LPhoton calls (pvol_set_surface_integrator_maps): the caustic estimate and,
        without the final gather, the same estimate over the indirect map.  Each map is None or (p[n,3], wi[n,3], alpha[n,30],
        n_paths); from_preprocess=True takes the caustic and the indirect store the last preprocess() kept instead.
        final_gather=True with a non-empty indirect map raises PVOL_E_UNSUPPORTED: the tile driver does not gather
        (radiance_gather_batch() does, for the caller's own rays)."""
        sp = abi.SurfaceParams()
        sp.n_used, sp.max_dist, sp.max_specular_depth, sp.final_gather = int(n_used), float(max_dist), int(max_specular_depth), int(bool(final_gather))
        sp.use_preprocess_store = int(bool(from_preprocess))
        ca, keep_c = photon_array(caustic)
        ia, keep_i = photon_array(indirect)
        _check(lib().pvol_set_surface_integrator_maps(self._h, C.byref(sp), C.byref(ca) if ca is not None else None,
                                                      C.byref(ia) if ia is not None else None), "pvol_set_surface_integrator_maps")
        del keep_c, keep_i

    def film_add_samples(self, film, d_image_xy, d_xyz, stride, n, d_pixels, hip_stream=0, window=None):
        if window is not None:
            _check(lib().pvol_film_add_samples_window_device(self._h, C.byref(film), C.byref(window), d_image_xy, d_xyz, stride, n, d_pixels, hip_stream),
                   "pvol_film_add_samples_window_device")
            return
        _check(lib().pvol_film_add_samples_device(self._h, C.byref(film), d_image_xy, d_xyz, stride, n, d_pixels, hip_stream),
               "pvol_film_add_samples_device")

    def film_resolve(self, film, d_pixels, d_rgb, hip_stream=0, window=None):
        if window is not None:
            _check(lib().pvol_film_resolve_window_device(self._h, C.byref(film), C.byref(window), d_pixels, d_rgb, hip_stream),
                   "pvol_film_resolve_window_device")
            return
        _check(lib().pvol_film_resolve_device(self._h, C.byref(film), d_pixels, d_rgb, hip_stream), "pvol_film_resolve_device")

    def li_single(self, ray, mt, mti):
        """Per-sample shim: ray is a length-1 RAY_DTYPE array, mt a uint32[624] array (updated in place)."""
        Lv = np.zeros(30, np.float32)
        T = np.zeros(30, np.float32)
        i = C.c_int32(int(mti))
        ray = np.ascontiguousarray(ray)
        _check(lib().pvol_li(self._h, ray.ctypes.data, mt.ctypes.data_as(_u32p), C.byref(i), Lv.ctypes.data_as(_f32p), T.ctypes.data_as(_f32p)),
               "pvol_li")
        return Lv, T, i.value

    def li_many(self, rays, mt, mti):
        """pvol_li_many: len(rays) independent per-sample calls in one batch, call i with the live state mt[i] (uint32[624]),
        mti[i].  Returns (Lv[n,30], T[n,30], mti[n], status[n]); mt is advanced in place.  Raises only for a batch-wide
        argument error: a call that failed on its own (PVOL_E_LIMIT) has its code in status and its state left as it was."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype == abi.RAY_DTYPE and mt.dtype == np.uint32 and mt.flags["C_CONTIGUOUS"]
        n = len(rays)
        assert mt.shape == (n, 624)
        mti = np.ascontiguousarray(mti, np.int32).copy()
        Lv = np.zeros((n, 30), np.float32)
        T = np.zeros((n, 30), np.float32)
        status = np.zeros(n, np.int32)
        rc = lib().pvol_li_many(self._h, rays.ctypes.data, n, mt.ctypes.data_as(_u32p), mti.ctypes.data_as(C.POINTER(C.c_int32)),
                                Lv.ctypes.data_as(_f32p), T.ctypes.data_as(_f32p), status.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != abi.PVOL_OK and not (status != abi.PVOL_OK).any():
            _check(rc, "pvol_li_many")
        return Lv, T, mti, status

    def set_li_coalescing(self, max_batch, max_wait_us=0):
        """Concurrent li_single (pvol_li) calls on this context are gathered into batches of up to max_batch (<= 1: off)."""
        _check(lib().pvol_set_li_coalescing(self._h, int(max_batch), int(max_wait_us)), "pvol_set_li_coalescing")

    def li_coalescing_stats(self, reset=False):
        v = (C.c_uint64 * 6)()
        _check(lib().pvol_get_li_coalescing_stats(self._h, v, int(reset)), "pvol_get_li_coalescing_stats")
        return dict(zip(["calls", "batches", "largest_batch", "queued_behind", "batches_redone", "calls_failed"], (int(x) for x in v)))

    def transmittance(self, rays, streams):
        rays = np.ascontiguousarray(rays)
        n = len(rays)
        out = np.zeros((n, 30), np.float32)
        _check(lib().pvol_transmittance_batch(self._h, rays.ctypes.data, n, streams.ctypes.data, len(streams), out.ctypes.data_as(_f32p)),
               "pvol_transmittance_batch")
        return out

    def enable_stats(self, on=True):
        _check(lib().pvol_enable_stats(self._h, int(on)), "pvol_enable_stats")

    def stats(self, reset=False):
        s = abi.Stats()
        _check(lib().pvol_get_stats(self._h, C.byref(s), int(reset)), "pvol_get_stats")
        return {k: int(getattr(s, k)) for k, _ in abi.Stats._fields_}

    def march_kernel_name(self):
        return lib().pvol_march_kernel_name(self._h).decode()

    def tile_kernel_name(self):
        """The form of the tile pre-pass the last render batch launched ("" if none ran)."""
        return lib().pvol_tile_kernel_name(self._h).decode()

    def tile_form_name(self):
        """"plain" or "general": which compilation of that kernel ran (pvol_tile_plain_gate; PVOL_TILE_GENERAL=1 keeps the general one)."""
        return lib().pvol_tile_form_name(self._h).decode()

    def kernel_time_ms(self, reset=False):
        avg = C.c_double()
        n = C.c_uint64()
        _check(lib().pvol_kernel_time_ms(self._h, C.byref(avg), C.byref(n), int(reset)), "pvol_kernel_time_ms")
        return avg.value, n.value


def gaussian_filter_table(xwidth=2.0, ywidth=2.0, alpha=2.0):
    t = np.zeros(256, np.float32)
    lib().pvol_gaussian_filter_table(xwidth, ywidth, alpha, t.ctypes.data_as(_f32p))
    return t


def sub_window(sampler, task):
    w = (C.c_int32 * 4)()
    lib().pvol_compute_sub_window(C.byref(sampler), task, w)
    return list(w)


def film_window_from_crop(film, crop):
    """pvol_film_window_from_crop: ImageFilm's pixel window of `crop` = (x0, x1, y0, y1) in [0, 1] (film/image.cpp:48-51).
    Pure host code: needs no GPU."""
    c = np.ascontiguousarray(crop, np.float32).reshape(-1)
    if c.size != 4:
        raise ValueError("cropwindow takes four numbers (x0 x1 y0 y1), got %d" % c.size)
    w = abi.FilmWindow()
    _check(lib().pvol_film_window_from_crop(C.byref(film), c.ctypes.data_as(_f32p), C.byref(w)), "pvol_film_window_from_crop")
    return w


def film_sample_extent(film, window=None):
    """pvol_film_sample_extent: ImageFilm::GetSampleExtent of the window (None: the whole frame) as [x_start, x_end, y_start, y_end].
    Pure host code: needs no GPU."""
    e = (C.c_int32 * 4)()
    _check(lib().pvol_film_sample_extent(C.byref(film), C.byref(window) if window is not None else None, e), "pvol_film_sample_extent")
    return list(e)


def render_sample_count(sampler, task_ids):
    ids = np.ascontiguousarray(task_ids, np.uint32)
    return int(lib().pvol_render_sample_count(C.byref(sampler), ids.ctypes.data_as(_u32p), len(ids)))
