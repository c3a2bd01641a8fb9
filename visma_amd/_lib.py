"""ctypes binding of the C ABI in include/visma_icp.h (libvisma_icp.so).

The library is the product: HIP kernels for gfx950 + the C++ host driver.
There is no Python or CPU implementation behind it -- if the shared library
is missing, or no GPU is visible when a context is created, this module
raises; it never falls back.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libvisma_icp.so")

NSTATS = 38
UNIQUE_ID_BYTES = 128
IPC_HANDLE_BYTES = 64
SOLVER_KABSCH, SOLVER_GN_EULER, SOLVER_GN_EXPMAP = 0, 1, 2
NN_AUTO, NN_BRUTE, NN_GRID = 0, 1, 2
OK = 0
ERR_NAMES = {1: "INVALID", 2: "NO_DEVICE", 3: "HIP", 4: "RCCL", 5: "STATE", 6: "ENGINE"}

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


class IcpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("visma_icp error %d (%s): %s" % (code, ERR_NAMES.get(code, "?"), msg))
        self.code = code


class CResult(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness", C.c_double),
                ("inlier_rmse", C.c_double), ("num_correspondences", C.c_int64),
                ("iterations", C.c_int32), ("nn_passes", C.c_int32)]


class CTiming(C.Structure):
    _fields_ = [("nn_ms", C.c_double), ("nn_launches", C.c_int64),
                ("reduce_ms", C.c_double), ("reduce_launches", C.c_int64),
                ("aux_ms", C.c_double), ("aux_launches", C.c_int64),
                ("grid_candidates", C.c_double), ("grid_candidates_27cell", C.c_double),
                ("tile_workgroups", C.c_double), ("tile_fallback_workgroups", C.c_double), ("tile_parts", C.c_double),
                ("tile_points", C.c_double), ("tile_rows", C.c_double), ("f64_reranks", C.c_double),
                ("tile_phase_cycles", C.c_double * 7), ("grid_certified", C.c_double),
                ("persist_launches", C.c_double), ("persist_passes", C.c_double), ("persist_ms", C.c_double),
                ("persist_aborts", C.c_double)]


class CPersistentInfo(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("enabled", C.c_int), ("last_loop_persistent", C.c_int), ("last_loop_passes", C.c_int),
                ("launches", C.c_double), ("passes", C.c_double), ("aborts", C.c_double), ("timeout_ms", C.c_double),
                ("cu_share", C.c_double), ("device_slots", C.c_int), ("reserved", C.c_int)]


class CProblem(C.Structure):
    _fields_ = [("src_xyz", _dp), ("ns", C.c_int64), ("tgt_xyz", _dp), ("nt", C.c_int64),
                ("init", C.c_double * 16), ("max_dist", C.c_double)]


class CPoseGraphEdge(C.Structure):
    """visma_icp_pose_graph_edge"""
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("transformation", C.c_double * 16),
                ("information", C.c_double * 36), ("uncertain", C.c_int32), ("confidence", C.c_double)]


class CGlobalOptimizationOption(C.Structure):
    """visma_icp_global_optimization_option"""
    _fields_ = [("max_correspondence_distance", C.c_double), ("edge_prune_threshold", C.c_double),
                ("preference_loop_closure", C.c_double), ("reference_node", C.c_int32)]


class COdometryOption(C.Structure):
    """visma_icp_odometry_option"""
    _fields_ = [("n_levels", C.c_int), ("iterations", C.c_int * 8), ("max_depth_diff", C.c_double), ("min_depth", C.c_double),
                ("max_depth", C.c_double)]


class COdometryResult(C.Structure):
    """visma_icp_odometry_result"""
    _fields_ = [("success", C.c_int), ("iterations", C.c_int), ("information_pairs", C.c_int64), ("pairs", C.POINTER(C.c_int64)),
                ("pairs_capacity", C.c_int)]


ODOMETRY_COLOR, ODOMETRY_HYBRID = 0, 1
# the images of a pyramid level (Context.odometry_image)
ODOMETRY_IMAGES = ("src_gray", "src_depth", "tgt_gray", "tgt_depth", "tgt_gray_dx", "tgt_gray_dy", "tgt_depth_dx", "tgt_depth_dy", "src_xyz")


def odometry_option(iterations=(20, 10, 5), max_depth_diff=0.03, min_depth=0.0, max_depth=4.0):
    """Open3D's OdometryOption: `iterations` per pyramid level, COARSEST level first (its length is the number of levels)."""
    o = COdometryOption()
    its = [int(i) for i in iterations]
    if not 1 <= len(its) <= 8:
        raise ValueError("1 .. 8 pyramid levels")
    o.n_levels = len(its)
    for i, n in enumerate(its):
        o.iterations[i] = n
    o.max_depth_diff, o.min_depth, o.max_depth = float(max_depth_diff), float(min_depth), float(max_depth)
    return o


class OdometryResult:
    """success, T (4 x 4, source camera -> target camera; the identity without success), information (6 x 6; zero without
    success), information_pairs (its K), pairs (the number of pairs of every iteration)"""

    def __init__(self, success, T, information, information_pairs, pairs):
        self.success, self.T, self.information = bool(success), T, information
        self.information_pairs, self.pairs = int(information_pairs), pairs

    def __iter__(self):                                  # (success, T, information): the reference's tuple
        return iter((self.success, self.T, self.information))


TSDF_COLOR_NONE, TSDF_COLOR_RGB8, TSDF_COLOR_GRAY32 = 0, 1, 2
_TSDF_COLOR_NAMES = {"none": TSDF_COLOR_NONE, "rgb8": TSDF_COLOR_RGB8, "gray32": TSDF_COLOR_GRAY32}


def _tsdf_color_type(color_type):
    return _TSDF_COLOR_NAMES[color_type.lower()] if isinstance(color_type, str) else int(color_type)


def _tsdf_color_image(color, color_type, shape):
    """the colour image of a frame as the C ABI takes it: h x w x 3 uint8 (RGB8), h x w fp32 (GRAY32), None otherwise"""
    if color_type == TSDF_COLOR_NONE or color is None:
        return None
    color = np.ascontiguousarray(color, dtype=np.uint8 if color_type == TSDF_COLOR_RGB8 else np.float32)
    if color.shape != (shape + (3,) if color_type == TSDF_COLOR_RGB8 else shape):
        raise ValueError("the colour image does not fit the depth image and the colour type")
    return color


class TsdfVolume:
    """A TSDF volume resident on the device (visma_icp_tsdf): Open3D's UniformTSDFVolume (Context.tsdf_uniform) or
    ScalableTSDFVolume (Context.tsdf_scalable; `resolution` is then a unit's and `length` its side).  Lives until close()
    or the context's end."""

    def __init__(self, ctx, handle, length, resolution, sdf_trunc, color_type, origin, scalable=False, voxel_length=None):
        self.ctx, self._v = ctx, handle
        self.length, self.resolution, self.sdf_trunc, self.color_type = float(length), int(resolution), float(sdf_trunc), color_type
        self.origin, self.scalable = origin, bool(scalable)
        self.voxel_length = self.length / self.resolution if voxel_length is None else float(voxel_length)

    def close(self):
        if self._v is not None and self.ctx._h:
            self.ctx._chk(self.ctx.L.visma_icp_tsdf_destroy(self.ctx._h, self._v))
        self._v = None

    def reset(self):
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_reset(self.ctx._h, self._v))

    def integrate(self, depth, color, intrinsic, extrinsic, intrinsic_size=None):
        """Integrate(): depth h x w fp32 (metres), color by the volume's colour type (h x w x 3 uint8 | h x w fp32 | None),
        intrinsic [fx, fy, cx, cy] of an image of intrinsic_size = (w, h) (default: the depth image's), extrinsic 4 x 4
        world -> camera.  depth (and color) may be resident Images (Context.image): the pixels are taken device to device
        (visma_icp_tsdf_integrate_images; intrinsic_size defaults to the depth image's size)."""
        if isinstance(depth, Image):
            if color is not None and not isinstance(color, Image):
                raise ValueError("a resident depth takes a resident colour image")
            k = _f64(intrinsic, (4,)); E = _f64(extrinsic, (16,))
            iw, ih = depth.info()[:2] if intrinsic_size is None else intrinsic_size
            self.ctx._chk(self.ctx.L.visma_icp_tsdf_integrate_images(self.ctx._h, self._v, depth._i, None if color is None else color._i,
                                                                     _p(k, _dp), int(iw), int(ih), _p(E, _dp)))
            return
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if depth.ndim != 2:
            raise ValueError("an h x w depth image")
        h, w = depth.shape
        color = _tsdf_color_image(color, self.color_type, (h, w))
        k = _f64(intrinsic, (4,)); E = _f64(extrinsic, (16,))
        iw, ih = (w, h) if intrinsic_size is None else intrinsic_size
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_integrate(self.ctx._h, self._v, w, h, _p(depth, _fp),
                                                          None if color is None else color.ctypes.data_as(C.c_void_p), _p(k, _dp),
                                                          int(iw), int(ih), _p(E, _dp)))

    def extract_point_cloud(self):
        """ExtractPointCloud() -> points, normals, colors (n x 3 f64; colors None for a volume without colour), in the
        reference's order: x, y, z, axis lexicographic."""
        n = C.c_int64(0)
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_extract_point_cloud(self.ctx._h, self._v, C.byref(n)))
        n = n.value
        pts, nrm = np.empty((n, 3)), np.empty((n, 3))
        col = np.empty((n, 3)) if self.color_type != TSDF_COLOR_NONE else None
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_get_point_cloud(self.ctx._h, self._v, _p(pts, _dp), _p(nrm, _dp),
                                                                None if col is None else _p(col, _dp), n))
        return pts, nrm, col

    def extract_voxel_point_cloud(self):
        """ExtractVoxelPointCloud() -> points, colors (n x 3 f64)"""
        n = C.c_int64(0)
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_extract_voxel_point_cloud(self.ctx._h, self._v, C.byref(n)))
        n = n.value
        pts, col = np.empty((n, 3)), np.empty((n, 3))
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_get_voxel_point_cloud(self.ctx._h, self._v, _p(pts, _dp), _p(col, _dp), n))
        return pts, col

    def extract_triangle_mesh(self):
        """ExtractTriangleMesh() -> vertices (n x 3 f64), colors (n x 3 f64, None for a volume without colour), triangles
        (m x 3 int32 vertex indices).  Vertices in ExtractPointCloud's order (x, y, z, axis of their voxel edge; a scalable
        volume's unit by unit), triangles cube by cube in that order (include/visma_icp.h: THE ORDER, THE CASE RULE)."""
        nv, nt = C.c_int64(0), C.c_int64(0)
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_extract_triangle_mesh(self.ctx._h, self._v, C.byref(nv), C.byref(nt)))
        nv, nt = nv.value, nt.value
        vtx = np.empty((nv, 3))
        col = np.empty((nv, 3)) if self.color_type != TSDF_COLOR_NONE else None
        tri = np.empty((nt, 3), np.int32)
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_get_triangle_mesh(self.ctx._h, self._v, _p(vtx, _dp), None if col is None else _p(col, _dp),
                                                                  _p(tri, _ip), nv, nt))
        return vtx, col, tri

    def triangle_mesh(self):
        """The last extracted mesh as a TriMesh, copied device to device (visma_icp_trimesh_from_tsdf): the volume's colours
        are its vertex colours, it has no normals.  Before an extract_triangle_mesh(): IcpError (state)."""
        m = C.c_void_p()
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_from_tsdf(self.ctx._h, self._v, C.byref(m)))
        return TriMesh(self.ctx, m)

    def point_cloud(self, voxel=False):
        """The last extract_point_cloud() (voxel=False) or extract_voxel_point_cloud() (True) as a Cloud, copied device to
        device (visma_icp_cloud_from_tsdf).  Before that extract, or after a frame or a reset: IcpError (state)."""
        c = C.c_void_p()
        self.ctx._chk(self.ctx.L.visma_icp_cloud_from_tsdf(self.ctx._h, self._v, int(bool(voxel)), C.byref(c)))
        return Cloud(self.ctx, c)

    def units(self):
        """The unit indices of a scalable volume (n x 3 int32) in lexicographic order: the order of its extractions."""
        n = C.c_int64(0)
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_get_units(self.ctx._h, self._v, None, 0, C.byref(n)))
        out = np.empty((max(n.value, 1), 3), np.int32)
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_get_units(self.ctx._h, self._v, _p(out, _ip), len(out), C.byref(n)))
        return out[:n.value].copy()

    def volume(self, unit=None):
        """-> tsdf, weight (R^3 fp32, voxel x R^2 + y R + z), color (R^3 x 3 fp32, or None) of a uniform volume, or of the
        unit with index `unit` (three ints) of a scalable one"""
        unit = None if unit is None else np.ascontiguousarray(unit, dtype=np.int32).reshape(3)
        n = self.resolution ** 3
        tsdf, weight = np.empty(n, np.float32), np.empty(n, np.float32)
        color = np.empty((n, 3), np.float32) if self.color_type != TSDF_COLOR_NONE else None
        self.ctx._chk(self.ctx.L.visma_icp_tsdf_get_volume(self.ctx._h, self._v, None if unit is None else _p(unit, _ip), _p(tsdf, _fp), _p(weight, _fp),
                                                           None if color is None else _p(color, _fp)))
        return tsdf, weight, color


TRIMESH_HAS_VERTEX_NORMALS, TRIMESH_HAS_VERTEX_COLORS, TRIMESH_HAS_TRIANGLE_NORMALS = 1, 2, 4


class TriMesh:
    """Open3D's TriangleMesh resident on the device (visma_icp_trimesh; Context.trimesh, TsdfVolume.triangle_mesh): normals,
    Purge, select, crop and Transform, every result the reference's bit for bit (include/visma_icp.h has the rules).  Lives
    until close() or the context's end; usable as a context manager."""

    def __init__(self, ctx, handle):
        self.ctx, self._m = ctx, handle

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        if self._m is not None and self.ctx._h:
            self.ctx._chk(self.ctx.L.visma_icp_trimesh_destroy(self.ctx._h, self._m))
        self._m = None

    def size(self):
        """-> nv, nt, has_flags (a mask of TRIMESH_HAS_*)"""
        nv, nt, f = C.c_int64(0), C.c_int64(0), C.c_int(0)
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_size(self._m, C.byref(nv), C.byref(nt), C.byref(f)))
        return nv.value, nt.value, f.value

    def get(self):
        """-> dict(vertices nv x 3 f64, triangles nt x 3 int32, vertex_normals, vertex_colors, triangle_normals: f64 rows, or
        None for what the mesh does not have)"""
        nv, nt, f = self.size()
        out = dict(vertices=np.empty((nv, 3)), triangles=np.empty((nt, 3), np.int32),
                   vertex_normals=np.empty((nv, 3)) if f & TRIMESH_HAS_VERTEX_NORMALS else None,
                   vertex_colors=np.empty((nv, 3)) if f & TRIMESH_HAS_VERTEX_COLORS else None,
                   triangle_normals=np.empty((nt, 3)) if f & TRIMESH_HAS_TRIANGLE_NORMALS else None)
        dp = lambda k: None if out[k] is None else _p(out[k], _dp)
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_get(self.ctx._h, self._m, dp("vertices"), dp("vertex_normals"), dp("vertex_colors"),
                                                       _p(out["triangles"], _ip), dp("triangle_normals"), nv, nt))
        return out

    def compute_triangle_normals(self, normalized=True):
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_compute_triangle_normals(self.ctx._h, self._m, int(bool(normalized))))

    def compute_vertex_normals(self, normalized=True):
        """ComputeVertexNormals: triangle normals the mesh has are used as they are, vertex normals it has are added onto"""
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_compute_vertex_normals(self.ctx._h, self._m, int(bool(normalized))))

    def normalize_normals(self):
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_normalize_normals(self.ctx._h, self._m))

    def _remove(self, call):
        r = C.c_int64(0)
        self.ctx._chk(call(self.ctx._h, self._m, C.byref(r)))
        return r.value

    def remove_duplicated_vertices(self):
        """-> the number of vertices removed"""
        return self._remove(self.ctx.L.visma_icp_trimesh_remove_duplicated_vertices)

    def remove_duplicated_triangles(self):
        return self._remove(self.ctx.L.visma_icp_trimesh_remove_duplicated_triangles)

    def remove_non_manifold_triangles(self):
        return self._remove(self.ctx.L.visma_icp_trimesh_remove_non_manifold_triangles)

    def remove_non_manifold_vertices(self):
        return self._remove(self.ctx.L.visma_icp_trimesh_remove_non_manifold_vertices)

    def purge(self):
        """Purge() -> the rows removed by its four steps: duplicated vertices, duplicated triangles, non-manifold triangles,
        non-manifold vertices"""
        r = (C.c_int64 * 4)()
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_purge(self.ctx._h, self._m, r))
        return tuple(int(v) for v in r)

    def select(self, indices):
        """SelectDownSample -> a new TriMesh, purged"""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        m = C.c_void_p()
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_select(self.ctx._h, self._m, _p(idx, C.POINTER(C.c_int64)), len(idx), C.byref(m)))
        return TriMesh(self.ctx, m)

    def crop(self, min_bound, max_bound):
        """CropTriangleMesh -> a new TriMesh, purged"""
        lo, hi = _f64(min_bound, (3,)), _f64(max_bound, (3,))
        m = C.c_void_p()
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_crop(self.ctx._h, self._m, _p(lo, _dp), _p(hi, _dp), C.byref(m)))
        return TriMesh(self.ctx, m)

    def transform(self, T):
        T = _f64(T, (16,))
        self.ctx._chk(self.ctx.L.visma_icp_trimesh_transform(self.ctx._h, self._m, _p(T, _dp)))

    def render(self, w, h, intrinsic, extrinsic=None, z_near=0.05, z_far=10.0, encoding="metric"):
        """The mesh seen by a pinhole camera (visma_icp_render has the rule) -> (depth, index, mask) Images: 1 x float32 depth
        (0 where nothing is drawn; encoding "depth_buffer": OpenGL's depth-buffer value, 1 where nothing is drawn), 1 x int32
        visible triangle (-1), 1 x uint8 mask (255 / 0).  intrinsic [fx, fy, cx, cy]; extrinsic world -> camera, 4 x 4."""
        k = _f64(intrinsic, (4,)); E = _f64(np.eye(4) if extrinsic is None else extrinsic, (16,))
        d, i, m = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ctx._chk(self.ctx.L.visma_icp_render(self.ctx._h, self._m, int(w), int(h), _p(k, _dp), _p(E, _dp), float(z_near), float(z_far),
                                                  _image_enum(encoding, RENDER_ENCODINGS), C.byref(d), C.byref(i), C.byref(m)))
        return Image(self.ctx, d), Image(self.ctx, i), Image(self.ctx, m)


CLOUD_HAS_NORMALS, CLOUD_HAS_COLORS = 1, 2


class Cloud:
    """Open3D's PointCloud resident on the device (visma_icp_cloud; Context.cloud, TsdfVolume.point_cloud): points and,
    optionally, normals and colours stay there between the steps of a pipeline (include/visma_icp.h has the rules and the
    deviations).  The operations that make a new cloud return a Cloud.  Lives until close() or the context's end; usable as
    a context manager."""

    def __init__(self, ctx, handle):
        self.ctx, self._c = ctx, handle

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _call(self, name, *args):
        self.ctx._chk(getattr(self.ctx.L, "visma_icp_cloud_" + name)(self.ctx._h, self._c, *args))

    def _new(self, name, *args):
        c = C.c_void_p()
        self._call(name, *args, C.byref(c))
        return Cloud(self.ctx, c)

    def close(self):
        if self._c is not None and self.ctx._h:
            self._call("destroy")
        self._c = None

    def size(self):
        """-> n, has_flags (a mask of CLOUD_HAS_*)"""
        n, f = C.c_int64(0), C.c_int(0)
        self.ctx._chk(self.ctx.L.visma_icp_cloud_size(self._c, C.byref(n), C.byref(f)))
        return n.value, f.value

    def __len__(self):
        return self.size()[0]

    def get(self):
        """-> dict(points n x 3 f64, normals, colors: n x 3 f64, or None for what the cloud does not have)"""
        n, f = self.size()
        out = dict(points=np.empty((n, 3)), normals=np.empty((n, 3)) if f & CLOUD_HAS_NORMALS else None,
                   colors=np.empty((n, 3)) if f & CLOUD_HAS_COLORS else None)
        dp = lambda k: None if out[k] is None else _p(out[k], _dp)
        self._call("get", dp("points"), dp("normals"), dp("colors"), n)
        return out

    def transform(self, T):
        self._call("transform", _p(_f64(T, (16,)), _dp))

    def normalize_normals(self):
        self._call("normalize_normals")

    def paint_uniform_color(self, rgb):
        self._call("paint_uniform_color", _p(_f64(rgb, (3,)), _dp))

    def append(self, other):
        """operator+=; other may be this cloud"""
        self._call("append", other._c)

    def bounds(self):
        """GetMinBound(), GetMaxBound() -> min (3), max (3)"""
        lo, hi = np.empty(3), np.empty(3)
        self._call("bounds", _p(lo, _dp), _p(hi, _dp))
        return lo, hi

    def select(self, indices):
        """SelectDownSample -> a new Cloud: the rows in the order of indices"""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        return self._new("select", _p(idx, C.POINTER(C.c_int64)), len(idx))

    def uniform_down_sample(self, every_k):
        """UniformDownSample -> a new Cloud: the rows 0, k, 2k, ... (every_k == 0: an empty one)"""
        return self._new("uniform_down_sample", int(every_k))

    def crop(self, min_bound, max_bound):
        """CropPointCloud -> a new Cloud"""
        lo, hi = _f64(min_bound, (3,)), _f64(max_bound, (3,))
        return self._new("crop", _p(lo, _dp), _p(hi, _dp))

    def voxel_down_sample(self, voxel_size):
        """VoxelDownSample -> a new Cloud: the rows of Context.voxel_down_sample"""
        return self._new("voxel_down_sample", float(voxel_size))

    def estimate_normals(self, knn=30, radius=None):
        """EstimateNormals in place: the normals of Context.estimate_normals for the same rows.  radius None: KNN(knn); knn
        None: Radius(radius); both: Hybrid.  Normals the cloud has keep their sign."""
        kind = 0 if radius is None else (1 if knn is None else 2)
        self._call("estimate_normals", kind, int(knn or 0), float(radius or 0.0))

    def orient_normals_to_align_with_direction(self, ref=(0.0, 0.0, 1.0)):
        self._call("orient_normals_to_align_with_direction", _p(_f64(ref, (3,)), _dp))

    def orient_normals_towards_camera_location(self, camera=(0.0, 0.0, 0.0)):
        self._call("orient_normals_towards_camera_location", _p(_f64(camera, (3,)), _dp))

    def mean_and_covariance(self):
        """ComputePointCloudMeanAndCovariance -> mean (3), covariance (3 x 3)"""
        mean, cov = np.empty(3), np.empty((3, 3))
        self._call("mean_and_covariance", _p(mean, _dp), _p(cov, _dp))
        return mean, cov

    def mahalanobis_distance(self):
        """ComputePointCloudMahalanobisDistance -> n f64"""
        out = np.empty(max(self.size()[0], 1))
        self._call("mahalanobis_distance", _p(out, _dp))
        return out[:self.size()[0]]


IMAGE_EQUAL, IMAGE_WEIGHTED = 0, 1
IMAGE_FILTERS = ("gaussian3", "gaussian5", "gaussian7", "sobel3dx", "sobel3dy")
RGBD_FORMATS = ("color_and_depth", "redwood", "tum", "sun", "nyu")
_IMAGE_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.float32}
RENDER_METRIC, RENDER_DEPTH_BUFFER = 0, 1
RENDER_ENCODINGS = ("metric", "depth_buffer")


def _image_enum(value, names):
    return names.index(value.lower()) if isinstance(value, str) else int(value)


class Image:
    """Open3D's Image resident on the device (visma_icp_image; Context.image, Context.rgbd): h x w pixels of 1 .. 4 channels
    of uint8, uint16 or float32 stay there between the steps of the RGB-D front end (include/visma_icp.h has the rules and
    the deviations).  The operations that make a new image return an Image; linear_transform and clip_intensity work in
    place.  Lives until close() or the context's end; usable as a context manager."""

    def __init__(self, ctx, handle):
        self.ctx, self._i = ctx, handle

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _call(self, name, *args):
        self.ctx._chk(getattr(self.ctx.L, "visma_icp_image_" + name)(self.ctx._h, self._i, *args))

    def _new(self, name, *args):
        i = C.c_void_p()
        self._call(name, *args, C.byref(i))
        return Image(self.ctx, i)

    def close(self):
        if self._i is not None and self.ctx._h:
            self._call("destroy")
        self._i = None

    def info(self):
        """-> width, height, channels, bytes per channel ((0, 0, 0, 0): the reference's empty Image)"""
        v = [C.c_int(0) for _ in range(4)]
        self.ctx._chk(self.ctx.L.visma_icp_image_info(self._i, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def is_int32(self):
        """True for the renderer's index image: one channel of four bytes that hold int32, not float"""
        v = C.c_int(0)
        self.ctx._chk(self.ctx.L.visma_icp_image_is_int32(self._i, C.byref(v)))
        return bool(v.value)

    def get(self):
        """-> h x w (one channel) or h x w x channels, uint8 / uint16 / float32 (int32: the renderer's index image); the empty
        Image: 0 x 0 uint8"""
        w, h, ch, bpc = self.info()
        out = np.empty((h, w) if ch <= 1 else (h, w, ch), np.int32 if self.is_int32() else _IMAGE_DTYPES.get(bpc, np.uint8))
        self._call("get", out.ctypes.data_as(C.c_void_p) if out.size else None, out.nbytes)
        return out

    def copy(self):
        return self._new("copy")

    def to_float(self, type=IMAGE_WEIGHTED):
        """CreateFloatImageFromImage; type IMAGE_EQUAL / IMAGE_WEIGHTED or "equal" / "weighted" """
        return self._new("to_float", _image_enum(type, ("equal", "weighted")))

    def depth_to_float(self, depth_scale=1000.0, depth_trunc=3.0):
        return self._new("depth_to_float", float(depth_scale), float(depth_trunc))

    def from_float(self, bytes=1):
        """CreateImageFromFloatImage<uint8_t> (1) / <uint16_t> (2); saturates outside the representable range"""
        return self._new("from_float", int(bytes))

    def filter(self, type):
        """FilterImage(type): an index or a name of IMAGE_FILTERS"""
        return self._new("filter", _image_enum(type, IMAGE_FILTERS))

    def filter_separable(self, dx, dy):
        dx, dy = _f64(dx, (-1,)), _f64(dy, (-1,))
        return self._new("filter_separable", _p(dx, _dp), len(dx), _p(dy, _dp), len(dy))

    def filter_horizontal(self, kernel):
        k = _f64(kernel, (-1,))
        return self._new("filter_horizontal", _p(k, _dp), len(k))

    def flip(self):
        """FlipImage: the transpose"""
        return self._new("flip")

    def downsample(self):
        return self._new("downsample")

    def dilate(self, half_kernel_size=1):
        return self._new("dilate", int(half_kernel_size))

    def linear_transform(self, scale, offset=0.0):
        self._call("linear_transform", float(scale), float(offset))

    def clip_intensity(self, min=0.0, max=1.0):
        self._call("clip_intensity", float(min), float(max))

    def pyramid(self, levels, with_gaussian_filter=True):
        """CreateImagePyramid -> a list of Images ([] for an image that is not 1 x float)"""
        levels = int(levels)
        out = (C.c_void_p * max(levels, 1))()
        self._call("pyramid", levels, int(bool(with_gaussian_filter)), out)
        return [Image(self.ctx, C.c_void_p(out[l])) for l in range(levels) if out[l]]

    def float_value_at(self, uv):
        """Image::FloatValueAt for n coordinates (n x 2: u, v) -> ok (n bool), value (n f64)"""
        uv = _f64(uv, (-1, 2))
        ok, value = np.zeros(max(len(uv), 1), np.uint8), np.zeros(max(len(uv), 1))
        self._call("float_value_at", _p(uv, _dp), len(uv), _p(ok, C.POINTER(C.c_uint8)), _p(value, _dp))
        return ok[:len(uv)].astype(bool), value[:len(uv)]


class KDTree:
    """A cloud resident on the device for neighbour queries (visma_icp_kdtree; Context.kdtree): Open3D's KDTreeFlann for
    batches of queries.  Every result is in the queries' order, a list ascending in (d2, index).  The grid behind a search is
    kept for the next call with the same radius or knn; another one rebuilds it.  Lives until close() or the context's end;
    usable as a context manager."""

    def __init__(self, ctx, handle, n):
        self.ctx, self._t, self.n = ctx, handle, int(n)

    def __len__(self):
        return self.n

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        if self._t is not None and self.ctx._h:
            self.ctx._chk(self.ctx.L.visma_icp_kdtree_destroy(self._t))
        self._t = None

    def _lists(self, call, queries, cap, *args):
        q = _f64(queries, (-1, 3))
        if int(cap) < 1:                                  # (no row can be shaped: the library's answer without its call)
            raise IcpError(1, "a list of at least one entry")
        rows = max(len(q), 1)
        idx, d2, cnt = np.empty((rows, int(cap)), np.int32), np.empty((rows, int(cap))), np.empty(rows, np.int32)
        self.ctx._chk(call(self._t, _p(q, _dp), len(q), *args, _p(idx, _ip), _p(d2, _dp), _p(cnt, _ip)))
        return idx[:len(q)], d2[:len(q)], cnt[:len(q)]

    def search_knn(self, queries, knn):
        """SearchKNN for every row of queries (nq x 3) -> idx (nq x knn int32, -1 behind a list), d2 (nq x knn, +inf behind
        it), cnt (nq): the min(knn, n) nearest."""
        return self._lists(self.ctx.L.visma_icp_kdtree_search_knn, queries, knn, int(knn))

    def search_hybrid(self, queries, radius, max_nn):
        """SearchHybrid: the max_nn nearest of those with d2 < (double)(float)(radius * radius); the layout of search_knn."""
        return self._lists(self.ctx.L.visma_icp_kdtree_search_hybrid, queries, max_nn, float(radius), int(max_nn))

    def search_radius(self, queries, radius):
        """SearchRadius: every neighbour with d2 < (double)(float)(radius * radius) -> offsets (nq + 1 int64), idx (total
        int32), d2 (total): query i owns [offsets[i], offsets[i + 1])."""
        q = _f64(queries, (-1, 3))
        offsets, total = np.zeros(len(q) + 1, np.int64), C.c_int64(0)
        self.ctx._chk(self.ctx.L.visma_icp_kdtree_search_radius(self._t, _p(q, _dp), len(q), float(radius),
                                                                _p(offsets, C.POINTER(C.c_int64)), C.byref(total)))
        idx, d2 = np.empty(max(total.value, 1), np.int32), np.empty(max(total.value, 1))
        self.ctx._chk(self.ctx.L.visma_icp_kdtree_get_radius_result(self._t, _p(idx, _ip), _p(d2, _dp)))
        return offsets, idx[:total.value], d2[:total.value]


class CColorMapOption(C.Structure):
    """visma_icp_color_map_option (Open3D's ColorMapOptmizationOption, field for field)"""
    _fields_ = [("non_rigid_camera_coordinate", C.c_int32), ("number_of_vertical_anchors", C.c_int32),
                ("non_rigid_anchor_point_weight", C.c_double), ("maximum_iteration", C.c_double), ("maximum_allowable_depth", C.c_double),
                ("depth_threshold_for_visiblity_check", C.c_double), ("depth_threshold_for_discontinuity_check", C.c_double),
                ("half_dilation_kernel_size_for_discontinuity_map", C.c_int32), ("reserved", C.c_int32)]


COLOR_MAP_IMAGES = ("gray", "dx", "dy", "mask")
COLOR_MAP_SUMS = 29
COLOR_MAP_CELL_SUMS = 121


def color_map_option(**fields):
    """The library's defaults (visma_icp_color_map_option_default: Open3D's) with `fields` on top, e.g. maximum_iteration=8."""
    o = CColorMapOption()
    load().visma_icp_color_map_option_default(C.byref(o))
    for k, v in fields.items():
        if k not in dict(CColorMapOption._fields_) or k == "reserved":
            raise TypeError("no such option: " + k)
        setattr(o, k, v)
    return o


class ColorMap:
    """A color map optimization resident on the device (visma_icp_color_map; Context.color_map): the staged calls of
    visma_icp.h.  Lives until close() or the context's end."""

    def __init__(self, ctx, handle, w, h, n_images):
        self.ctx, self._m, self.w, self.h, self.n_images, self.n_vertices = ctx, handle, int(w), int(h), int(n_images), 0
        self._shape = None

    def _call(self, name, *args):
        self.ctx._chk(getattr(self.ctx.L, "visma_icp_color_map_" + name)(self.ctx._h, self._m, *args))

    def close(self):
        if self._m is not None and self.ctx._h:
            self._call("destroy")
        self._m = None

    def set_image(self, i, depth, color, extrinsic):
        """frame i: depth h x w fp32 (metres), color h x w x 3 uint8, extrinsic 4 x 4 world -> camera"""
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        color = np.ascontiguousarray(color, dtype=np.uint8)
        if depth.shape != (self.h, self.w) or color.ndim != 3 or color.shape[:2] != (self.h, self.w):
            raise ValueError("the images do not fit the color map's size")
        E = _f64(extrinsic, (16,))
        self._call("set_image", int(i), _p(depth, _fp), color.ctypes.data_as(C.POINTER(C.c_uint8)), int(color.shape[2]), _p(E, _dp))

    def set_vertices(self, vertices):
        v = _f64(vertices, (-1, 3))
        self._call("set_vertices", _p(v, _dp), len(v))
        self.n_vertices = len(v)

    def prepare(self):
        """images, masks, visibility -> the visible vertex count of every camera (int64)"""
        counts = np.zeros(self.n_images, np.int64)
        self._call("prepare", counts.ctypes.data_as(C.POINTER(C.c_int64)))
        return counts

    def image(self, i, which):
        """which: "gray" | "dx" | "dy" (h x w fp32) | "mask" (h x w uint8)"""
        k = COLOR_MAP_IMAGES.index(which) if isinstance(which, str) else int(which)
        out = np.empty((self.h, self.w), np.uint8 if k == 3 else np.float32)
        self._call("get_image", int(i), k, out.ctypes.data_as(C.c_void_p))
        return out

    def visible(self, i):
        """camera i's visible vertices, ascending (int32)"""
        n = C.c_int64(0)
        self._call("get_visible", int(i), None, 0, C.byref(n))
        out = np.empty(max(n.value, 1), np.int32)
        self._call("get_visible", int(i), _p(out, _ip), len(out), C.byref(n))
        return out[:n.value].copy()

    def proxy(self):
        out = np.empty(self.n_vertices)
        self._call("get_proxy", _p(out, _dp), self.n_vertices)
        return out

    def sums(self):
        """n_images x 29 at the current poses: JJ's 21 upper entries row by row, Jb[6], rr, count; no pose moves"""
        out = np.empty((self.n_images, COLOR_MAP_SUMS))
        self._call("sums", _p(out, _dp))
        return out

    def step(self):
        """one iteration -> rr (n_images f64), count (n_images int64) of the poses before it"""
        rr, count = np.empty(self.n_images), np.empty(self.n_images, np.int64)
        self._call("step", _p(rr, _dp), count.ctypes.data_as(C.POINTER(C.c_int64)))
        return rr, count

    def run(self, k=-1):
        """k iterations (default: the option's maximum_iteration) -> the residual of every iteration"""
        out = np.empty(max(int(k), 0)) if k >= 0 else None
        self._call("run", int(k), None if out is None else _p(out, _dp))
        return out

    def extrinsics(self):
        out = np.empty((self.n_images, 4, 4))
        self._call("get_extrinsics", _p(out, _dp))
        return out

    def set_extrinsics(self, extrinsics):
        E = _f64(extrinsics, (self.n_images * 16,))
        self._call("set_extrinsics", _p(E, _dp))

    def colors(self):
        out = np.empty((self.n_vertices, 3))
        self._call("get_colors", _p(out, _dp), self.n_vertices)
        return out

    # ---- a non-rigid map (Context.color_map_non_rigid) alone ----
    def anchor_shape(self):
        """-> (anchor_w, anchor_h, anchor_step)"""
        if self._shape is None:
            aw, ah, step = C.c_int(0), C.c_int(0), C.c_double(0.0)
            self._call("get_anchor_shape", C.byref(aw), C.byref(ah), C.byref(step))
            self._shape = (aw.value, ah.value, step.value)
        return self._shape

    def flow(self):
        """n_images x (anchor_w anchor_h 2): entry (i + j anchor_w) 2 + {0, 1} is where anchor (i, j) points"""
        aw, ah, _ = self.anchor_shape()
        out = np.empty((self.n_images, aw * ah * 2))
        self._call("get_flow", _p(out, _dp))
        return out

    def set_flow(self, flow):
        aw, ah, _ = self.anchor_shape()
        f = _f64(flow, (self.n_images * aw * ah * 2,))
        self._call("set_flow", _p(f, _dp))

    def cell_sums(self):
        """n_images x cells x 121 at the current poses and fields (cell ii + jj (anchor_w - 1)); nothing moves"""
        aw, ah, _ = self.anchor_shape()
        out = np.empty((self.n_images, (aw - 1) * (ah - 1), COLOR_MAP_CELL_SUMS))
        self._call("cell_sums", _p(out, _dp))
        return out

    def step_non_rigid(self):
        """one iteration -> rr, rr_reg (n_images f64), count (n_images int64) of the state before it"""
        rr, reg, count = np.empty(self.n_images), np.empty(self.n_images), np.empty(self.n_images, np.int64)
        self._call("step_non_rigid", _p(rr, _dp), _p(reg, _dp), count.ctypes.data_as(C.POINTER(C.c_int64)))
        return rr, reg, count


def color_map_solve_non_rigid(anchor_w, anchor_h, cell_sums, n_vertex, weight, flow, flow_init):
    """visma_icp_color_map_solve_non_rigid (host only): one camera's cell rows -> (x of 6 + anchor_w anchor_h 2, rr_reg, kept)"""
    aw, ah = int(anchor_w), int(anchor_h)
    if aw < 2 or ah < 2 or aw * ah > 8192:
        raise IcpError(1, "color_map_solve_non_rigid: bad anchor shape")
    rows = _f64(cell_sums, ((aw - 1) * (ah - 1) * COLOR_MAP_CELL_SUMS,))
    f, f0 = _f64(flow, (aw * ah * 2,)), _f64(flow_init, (aw * ah * 2,))
    x, reg, kept = np.empty(6 + aw * ah * 2), C.c_double(0.0), C.c_int(0)
    rc = load().visma_icp_color_map_solve_non_rigid(aw, ah, _p(rows, _dp), int(n_vertex), float(weight), _p(f, _dp), _p(f0, _dp),
                                                    _p(x, _dp), C.byref(reg), C.byref(kept))
    if rc != 0:
        raise IcpError(rc, "color_map_solve_non_rigid: bad arguments")
    return x, reg.value, bool(kept.value)


class CGlobalOptimizationCriteria(C.Structure):
    """visma_icp_global_optimization_criteria"""
    _fields_ = [("max_iteration", C.c_int32), ("min_relative_increment", C.c_double),
                ("min_relative_residual_increment", C.c_double), ("min_right_term", C.c_double), ("min_residual", C.c_double),
                ("max_iteration_lm", C.c_int32), ("upper_scale_factor", C.c_double), ("lower_scale_factor", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, C.c_int)
MINREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_int64)
ENG_SET = C.CFUNCTYPE(C.c_int, C.c_void_p, _fp, C.c_int64)
ENG_NN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, C.c_double)
ENG_REDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, _dp, C.c_int, _dp)
ENG_CORR = C.CFUNCTYPE(C.c_int, C.c_void_p, _ip, _fp)


class CMeshSource(C.Structure):
    _fields_ = [("V", C.POINTER(C.c_double)), ("nv", C.c_int64), ("F", C.POINTER(C.c_int32)), ("nf", C.c_int64),
                ("samples", C.c_int64), ("model_to_scene", C.POINTER(C.c_double))]


class CCorpusItem(C.Structure):
    _fields_ = [("model_xyz", C.POINTER(C.c_double)), ("n_model", C.c_int64),
                ("scene_xyz", C.POINTER(C.c_double)), ("n_scene", C.c_int64)]


class CCorpusParams(C.Structure):
    _fields_ = [("level", C.c_int), ("max_dist", C.c_double), ("max_iter", C.c_int), ("rel_fitness", C.c_double),
                ("rel_rmse", C.c_double), ("solver", C.c_int), ("chunk", C.c_int)]


class CCorpusResult(C.Structure):
    _fields_ = [("best", CResult), ("best_level", C.c_int32), ("device", C.c_int32), ("iterations_all_starts", C.c_int64)]


class CEngine(C.Structure):
    _fields_ = [("set_source", ENG_SET), ("set_target", ENG_SET),
                ("set_target_normals", ENG_SET), ("nn_pass", ENG_NN),
                ("reduce", ENG_REDUCE), ("get_correspondences", ENG_CORR)]


_lib = None


_seams = None


def load_seams():
    """The side build with the test seam visma_icp_create_with_engine (and the experiments that lost): what the
    CPU suite drives the host loop through.  Never the product library."""
    global _seams
    if _seams is None:
        from . import build
        _seams = _bind(C.CDLL(build.build_experiments()))
    return _seams


def load():
    """Load libvisma_icp.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    lib_path = os.environ.get("VISMA_ICP_LIB", LIB_PATH)     # (experiments: an alternative build of the same library)
    if not os.path.exists(lib_path):
        raise ImportError(
            "%s is missing: build it with `python -m visma_amd.build` (hipcc, gfx950). "
            "visma_amd has no non-HIP implementation." % lib_path)
    _lib = _bind(C.CDLL(lib_path))
    return _lib


def _bind(L):
    L.visma_icp_last_error.restype = C.c_char_p
    L.visma_icp_last_error.argtypes = [C.c_void_p]
    L.visma_icp_version.restype = C.c_char_p
    L.visma_icp_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    if hasattr(L, "visma_icp_create_with_engine"):
        L.visma_icp_create_with_engine.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CEngine), C.c_void_p]
    L.visma_icp_destroy.argtypes = [C.c_void_p]
    L.visma_icp_set_clouds_f64.argtypes = [C.c_void_p, _dp, C.c_int64, C.c_int, _dp, C.c_int64, C.c_int]
    L.visma_icp_set_clouds_f64_voxel_target.argtypes = [C.c_void_p, _dp, C.c_int64, C.c_int, _dp, C.c_int64, C.c_int,
                                                        C.c_double, C.POINTER(C.c_int64)]
    L.visma_icp_get_voxel_target.argtypes = [C.c_void_p, _dp, C.c_int64]
    L.visma_icp_set_clouds_meshes_f64.argtypes = [C.c_void_p, C.POINTER(CMeshSource), C.c_int, C.c_int, C.c_uint64, _dp,
                                                  C.c_int64, C.c_int, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.visma_icp_get_mesh_source.argtypes = [C.c_void_p, _dp, C.c_int64]
    L.visma_icp_set_radius_hint.argtypes = [C.c_void_p, C.c_double]
    L.visma_icp_set_target.argtypes = [C.c_void_p, _fp, C.c_int64, C.c_int]
    L.visma_icp_set_source.argtypes = [C.c_void_p, _fp, C.c_int64, C.c_int]
    L.visma_icp_set_target_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.visma_icp_set_source_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.visma_icp_set_target_normals_f64.argtypes = [C.c_void_p, _dp, C.c_int64, C.c_int]
    L.visma_icp_get_search_kernel_used.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.visma_icp_forget_winners.argtypes = [C.c_void_p]
    L.visma_icp_run_batch_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CProblem), C.c_int, C.c_int, C.c_double,
                                            C.c_double, C.c_int, C.POINTER(CResult), C.c_char_p, C.c_size_t]
    L.visma_icp_run_corpus.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CCorpusItem), C.c_int64,
                                       C.POINTER(CCorpusParams), C.POINTER(C.c_int64), C.POINTER(CCorpusResult),
                                       C.c_char_p, C.c_size_t]
    L.visma_icp_nn_pass.argtypes = [C.c_void_p, _dp, C.c_double]
    L.visma_icp_reduce.argtypes = [C.c_void_p, _dp]
    L.visma_icp_get_correspondences.argtypes = [C.c_void_p, _ip, _ip, _fp, C.POINTER(C.c_int64)]
    L.visma_icp_solve_from_stats.argtypes = [_dp, C.c_int, C.c_int, _dp]
    L.visma_icp_run.argtypes = [C.c_void_p, _dp, C.c_double, C.c_int, C.c_double, C.c_double,
                                C.c_int, C.c_int, C.POINTER(CResult)]
    L.visma_icp_iterate.argtypes = [C.c_void_p, _dp, C.c_double, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(CResult)]
    L.visma_icp_run_point_to_plane.argtypes = [C.c_void_p, _dp, C.c_double, C.c_int, C.c_double,
                                               C.c_double, C.POINTER(CResult)]
    L.visma_icp_run_yaw_sweep.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double,
                                          C.c_double, C.c_int, C.POINTER(CResult),
                                          C.POINTER(C.c_int), C.POINTER(CResult)]
    L.visma_icp_estimate_normals.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int, C.c_int, C.c_double, _dp]
    L.visma_icp_run_batch_point_to_plane.argtypes = [C.c_void_p, C.POINTER(CProblem), C.POINTER(_dp), C.c_int, C.c_int,
                                                     C.c_double, C.c_double, C.POINTER(CResult)]
    L.visma_icp_run_batch.argtypes = [C.c_void_p, C.POINTER(CProblem), C.c_int, C.c_int,
                                      C.c_double, C.c_double, C.c_int, C.POINTER(CResult)]
    L.visma_icp_voxel_down_sample.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, C.c_double, _dp, _dp,
                                              _dp, C.POINTER(C.c_int64)]
    L.visma_icp_sample_mesh.argtypes = [C.c_void_p, _dp, C.c_int64, _ip, C.c_int64, C.c_int64, C.c_int,
                                        C.c_uint64, _dp, _dp, C.POINTER(C.c_int64)]
    L.visma_icp_point_mesh_distance.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int64, _ip, C.c_int64,
                                                _dp, _ip, _dp]
    L.visma_icp_last_mesh_kernel_ms.argtypes = [C.c_void_p, _dp, _dp]
    L.visma_icp_set_mesh_search.argtypes = [C.c_void_p, C.c_int]
    L.visma_icp_error_metric.argtypes = [_dp, C.c_int64, _dp]
    L.visma_icp_measure_surface_error.argtypes = [C.c_void_p, _dp, C.c_int64, _ip, C.c_int64, _dp, C.c_int64,
                                                  _ip, C.c_int64, C.c_int64, C.c_int, C.c_uint64, _dp]
    L.visma_icp_set_target_shard.argtypes = [C.c_void_p, C.c_int64, C.c_int64, _dp]
    L.visma_icp_set_minreduce.argtypes = [C.c_void_p, MINREDUCE_FN, C.c_void_p]
    L.visma_icp_set_search_precision.argtypes = [C.c_void_p, C.c_int]
    L.visma_icp_get_search_precision_used.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.visma_icp_set_nn_mode.argtypes = [C.c_void_p, C.c_int]
    L.visma_icp_get_nn_mode_used.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.visma_icp_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.visma_icp_set_device_loop.argtypes = [C.c_void_p, C.c_int]
    L.visma_icp_set_persistent.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.visma_icp_test_stall_command.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.visma_icp_get_sweep_info.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "visma_icp_set_ring_search"):          # (A/B runs load older builds through VISMA_ICP_LIB)
        L.visma_icp_set_ring_search.argtypes = [C.c_void_p, C.c_int]
        L.visma_icp_get_ring_search.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "visma_icp_set_rotation_axis"):        # (A/B runs load older builds through VISMA_ICP_LIB)
        L.visma_icp_set_rotation_axis.argtypes = [C.c_void_p, _dp]
        L.visma_icp_get_rotation_axis.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_int)]
        L.visma_icp_solve_from_stats_axis.argtypes = [_dp, C.c_int, _dp, _dp]
    if hasattr(L, "visma_icp_point_cloud_distance"):     # (A/B runs load older builds through VISMA_ICP_LIB)
        L.visma_icp_point_cloud_distance.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int64, _dp]
        L.visma_icp_nearest_neighbor_distance.argtypes = [C.c_void_p, _dp, C.c_int64, _dp]
    if hasattr(L, "visma_icp_run_trimmed"):              # (A/B runs load older builds through VISMA_ICP_LIB)
        _tp = C.POINTER(CTrimInfo)
        L.visma_icp_reduce_trimmed.argtypes = [C.c_void_p, C.c_double, _dp, _tp]
        L.visma_icp_run_trimmed.argtypes = [C.c_void_p, _dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                            C.c_int, C.c_int, C.POINTER(CResult), _tp]
        L.visma_icp_run_yaw_sweep_trimmed.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                                      C.c_double, C.c_int, C.POINTER(CResult), C.POINTER(C.c_int),
                                                      C.POINTER(CResult), _tp, _tp]
        L.visma_icp_get_kept_mask.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
    if hasattr(L, "visma_icp_run_robust"):               # (A/B runs load older builds through VISMA_ICP_LIB)
        _rc, _ri = C.POINTER(CRobust), C.POINTER(CRobustInfo)
        L.visma_icp_reduce_robust.argtypes = [C.c_void_p, _rc, C.c_int, _dp, _ri]
        L.visma_icp_run_robust.argtypes = [C.c_void_p, _dp, C.c_double, _rc, C.c_int, C.c_int, C.c_double, C.c_double,
                                           C.c_int, C.POINTER(CResult), _ri]
        L.visma_icp_run_yaw_sweep_robust.argtypes = [C.c_void_p, C.c_int, C.c_double, _rc, C.c_int, C.c_int, C.c_double,
                                                     C.c_double, C.POINTER(CResult), C.POINTER(C.c_int),
                                                     C.POINTER(CResult), _ri, _ri]
        L.visma_icp_get_pair_weights.argtypes = [C.c_void_p, _dp]
    if hasattr(L, "visma_icp_run_gicp"):                 # (A/B runs load older builds through VISMA_ICP_LIB)
        _gi = C.POINTER(CGicpInfo)
        L.visma_icp_set_source_normals_f64.argtypes = [C.c_void_p, _dp, C.c_int64, C.c_int]
        L.visma_icp_reduce_gicp.argtypes = [C.c_void_p, C.c_double, _dp, _gi]
        L.visma_icp_run_gicp.argtypes = [C.c_void_p, _dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                         C.POINTER(CResult), _gi]
        L.visma_icp_run_yaw_sweep_gicp.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                                   C.c_double, C.POINTER(CResult), C.POINTER(C.c_int), C.POINTER(CResult),
                                                   _gi, _gi]
    if hasattr(L, "visma_icp_run_colored"):              # (A/B runs load older builds through VISMA_ICP_LIB)
        _ci = C.POINTER(CColoredInfo)
        L.visma_icp_set_source_colors_f64.argtypes = [C.c_void_p, _dp, C.c_int64, C.c_int]
        L.visma_icp_set_target_colors_f64.argtypes = [C.c_void_p, _dp, C.c_int64, C.c_int]
        L.visma_icp_prepare_colored.argtypes = [C.c_void_p, C.c_double, C.c_int]
        L.visma_icp_get_color_gradient.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.visma_icp_reduce_colored.argtypes = [C.c_void_p, C.c_double, _dp, _ci]
        L.visma_icp_run_colored.argtypes = [C.c_void_p, _dp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                            C.POINTER(CResult), _ci]
        L.visma_icp_color_gradient.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, C.c_double, C.c_int, _dp]
    if hasattr(L, "visma_icp_fast_global_registration"):  # (A/B runs load older builds through VISMA_ICP_LIB)
        _fo, _fi = C.POINTER(CFgrOption), C.POINTER(CFgrInfo)
        L.visma_icp_compute_fpfh.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int, C.c_int, C.c_double, _dp]
        L.visma_icp_compute_fpfh_probe.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int, C.c_int, C.c_double, _dp, C.c_int, _dp]
        L.visma_icp_match_features.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int64, C.c_int, _ip, _dp]
        L.visma_icp_match_features_probe.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int64, C.c_int, _ip, _dp, _dp]
        L.visma_icp_fgr_correspondences.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, C.c_int64, _dp, _fo, C.c_uint64, _ip,
                                                    C.c_int64, _ip, _ip, C.c_int64, C.POINTER(C.c_int64), _fi]
        L.visma_icp_fgr_optimize.argtypes = [_dp, C.c_int64, _dp, C.c_int64, _ip, _ip, C.c_int64, _fo, _dp, _dp]
        L.visma_icp_fast_global_registration.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, C.c_int64, _dp, _fo, C.c_uint64,
                                                         _ip, C.c_int64, _dp, _fi]
    if hasattr(L, "visma_icp_registration_ransac_feature_matching"):
        _ro, _ri, _bp = C.POINTER(CRansacOption), C.POINTER(CRansacInfo), C.POINTER(C.c_int8)
        hyp = [_dp, C.c_int64, _dp, C.c_int64, _dp, _dp, _ip, _ip, C.c_int64, _ro, C.c_uint64, _ip, C.c_int64, C.c_int64, _bp, _dp]
        L.visma_icp_ransac_hypotheses.argtypes = [C.c_void_p] + hyp
        L.visma_icp_ransac_hypotheses_host.argtypes = hyp
        L.visma_icp_ransac_hypotheses_probe.argtypes = [C.c_void_p] + hyp[:11] + [C.c_int64, C.POINTER(C.c_int64), _dp]
        L.visma_icp_registration_ransac_feature_matching.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, _dp, C.c_int64, _dp, C.c_int, _dp,
                                                                     _dp, C.c_double, _ro, C.c_uint64, _ip, C.c_int64,
                                                                     C.POINTER(CResult), _ri]
        L.visma_icp_registration_ransac_correspondence.argtypes = [C.c_void_p, _dp, C.c_int64, _dp, C.c_int64, _ip, _ip, C.c_int64,
                                                                   C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint64, _ip, C.c_int64,
                                                                   C.POINTER(CResult), _ri]
    if hasattr(L, "visma_icp_information_matrix"):       # (A/B runs load older builds through VISMA_ICP_LIB)
        _ep = C.POINTER(CPoseGraphEdge)
        L.visma_icp_information_matrix.argtypes = [C.c_void_p, _dp, C.c_double, _dp, C.POINTER(C.c_int64)]
        L.visma_icp_reduce_information.argtypes = [C.c_void_p, _dp]
        L.visma_icp_information_matrices.argtypes = [C.c_void_p, C.POINTER(CProblem), C.c_int, _dp, C.POINTER(C.c_int64)]
        L.visma_icp_global_optimization_option_clamp.argtypes = [C.POINTER(CGlobalOptimizationOption)]
        L.visma_icp_global_optimization_criteria_clamp.argtypes = [C.POINTER(CGlobalOptimizationCriteria)]
        L.visma_icp_pose_graph_validate.argtypes = [C.c_int, _ep, C.c_int]
        L.visma_icp_pose_graph_zeta.argtypes = [_dp, C.c_int, _ep, C.c_int, _dp]
        L.visma_icp_pose_graph_linear_system.argtypes = [_dp, C.c_int, _ep, C.c_int, _dp, _dp]
        L.visma_icp_global_optimization.argtypes = [_dp, C.c_int, _ep, C.POINTER(C.c_int), C.c_int,
                                                    C.POINTER(CGlobalOptimizationCriteria), C.POINTER(CGlobalOptimizationOption)]
        L.visma_icp_pose_graph_optimize.argtypes = [_dp, C.c_int, _ep, C.c_int, C.c_int,
                                                    C.POINTER(CGlobalOptimizationCriteria), C.POINTER(CGlobalOptimizationOption)]
        L.visma_icp_get_cloud_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(L, "visma_icp_rgbd_odometry"):            # (A/B runs load older builds through VISMA_ICP_LIB)
        _oo, _i64 = C.POINTER(COdometryOption), C.POINTER(C.c_int64)
        frames = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _dp, _dp]
        L.visma_icp_odometry_option_default.argtypes = [_oo]
        L.visma_icp_rgbd_odometry.argtypes = frames + [C.c_int, _oo, _dp, _dp, C.POINTER(COdometryResult)]
        L.visma_icp_odometry_prepare.argtypes = frames + [_oo]
        L.visma_icp_odometry_get_image.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp]
        L.visma_icp_odometry_correspondences.argtypes = [C.c_void_p, C.c_int, _dp, _ip, _i64]
        L.visma_icp_odometry_step.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int, _dp, _i64, _dp]
        L.visma_icp_odometry_information.argtypes = [C.c_void_p, _dp, _dp, _i64]
    if hasattr(L, "visma_icp_tsdf_create_uniform"):      # (A/B runs load older builds through VISMA_ICP_LIB)
        _i64, _vp = C.POINTER(C.c_int64), C.c_void_p
        L.visma_icp_tsdf_create_uniform.argtypes = [_vp, C.c_double, C.c_int, C.c_double, C.c_int, _dp, C.POINTER(_vp)]
        L.visma_icp_tsdf_destroy.argtypes = [_vp, _vp]
        L.visma_icp_tsdf_reset.argtypes = [_vp, _vp]
        L.visma_icp_tsdf_integrate.argtypes = [_vp, _vp, C.c_int, C.c_int, _fp, _vp, _dp, C.c_int, C.c_int, _dp]
        L.visma_icp_tsdf_extract_point_cloud.argtypes = [_vp, _vp, _i64]
        L.visma_icp_tsdf_get_point_cloud.argtypes = [_vp, _vp, _dp, _dp, _dp, C.c_int64]
        L.visma_icp_tsdf_extract_voxel_point_cloud.argtypes = [_vp, _vp, _i64]
        L.visma_icp_tsdf_get_voxel_point_cloud.argtypes = [_vp, _vp, _dp, _dp, C.c_int64]
        L.visma_icp_tsdf_get_volume.argtypes = [_vp, _vp, _ip, _fp, _fp, _fp]
        L.visma_icp_tsdf_create_scalable.argtypes = [_vp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]
        L.visma_icp_tsdf_get_units.argtypes = [_vp, _vp, _ip, C.c_int64, _i64]
        L.visma_icp_point_cloud_from_depth.argtypes = [_vp, C.c_int, C.c_int, _fp, _dp, _dp, C.c_int, _dp, C.c_int64, _i64]
        L.visma_icp_point_cloud_from_rgbd.argtypes = [_vp, C.c_int, C.c_int, _fp, _vp, C.c_int, _dp, _dp, _dp, _dp, C.c_int64, _i64]
    if hasattr(L, "visma_icp_tsdf_extract_triangle_mesh"):   # (A/B runs load older builds through VISMA_ICP_LIB)
        _i64, _vp = C.POINTER(C.c_int64), C.c_void_p
        L.visma_icp_tsdf_extract_triangle_mesh.argtypes = [_vp, _vp, _i64, _i64]
        L.visma_icp_tsdf_get_triangle_mesh.argtypes = [_vp, _vp, _dp, _dp, _ip, C.c_int64, C.c_int64]
        L.visma_icp_marching_cubes_case.argtypes = [C.c_int, _ip, C.POINTER(C.c_int)]
    if hasattr(L, "visma_icp_kdtree_create"):            # (A/B runs load older builds through VISMA_ICP_LIB)
        _i64, _vp = C.POINTER(C.c_int64), C.c_void_p
        L.visma_icp_kdtree_create.argtypes = [_vp, _dp, C.c_int64, C.POINTER(_vp)]
        L.visma_icp_kdtree_destroy.argtypes = [_vp]
        L.visma_icp_kdtree_size.argtypes = [_vp]
        L.visma_icp_kdtree_size.restype = C.c_int64
        L.visma_icp_kdtree_search_knn.argtypes = [_vp, _dp, C.c_int64, C.c_int, _ip, _dp, _ip]
        L.visma_icp_kdtree_search_hybrid.argtypes = [_vp, _dp, C.c_int64, C.c_double, C.c_int, _ip, _dp, _ip]
        L.visma_icp_kdtree_search_radius.argtypes = [_vp, _dp, C.c_int64, C.c_double, _i64, _i64]
        L.visma_icp_kdtree_get_radius_result.argtypes = [_vp, _ip, _dp]
    if hasattr(L, "visma_icp_trimesh_create"):           # (A/B runs load older builds through VISMA_ICP_LIB)
        _i64, _vp = C.POINTER(C.c_int64), C.c_void_p
        L.visma_icp_trimesh_create.argtypes = [_vp, _dp, C.c_int64, _dp, _dp, _ip, C.c_int64, _dp, C.POINTER(_vp)]
        L.visma_icp_trimesh_from_tsdf.argtypes = [_vp, _vp, C.POINTER(_vp)]
        L.visma_icp_trimesh_destroy.argtypes = [_vp, _vp]
        L.visma_icp_trimesh_size.argtypes = [_vp, _i64, _i64, C.POINTER(C.c_int)]
        L.visma_icp_trimesh_get.argtypes = [_vp, _vp, _dp, _dp, _dp, _ip, _dp, C.c_int64, C.c_int64]
        for name in ("compute_triangle_normals", "compute_vertex_normals"):
            getattr(L, "visma_icp_trimesh_" + name).argtypes = [_vp, _vp, C.c_int]
        L.visma_icp_trimesh_normalize_normals.argtypes = [_vp, _vp]
        for name in ("remove_duplicated_vertices", "remove_duplicated_triangles", "remove_non_manifold_triangles",
                     "remove_non_manifold_vertices", "purge"):
            getattr(L, "visma_icp_trimesh_" + name).argtypes = [_vp, _vp, _i64]
        L.visma_icp_trimesh_select.argtypes = [_vp, _vp, _i64, C.c_int64, C.POINTER(_vp)]
        L.visma_icp_trimesh_crop.argtypes = [_vp, _vp, _dp, _dp, C.POINTER(_vp)]
        L.visma_icp_trimesh_transform.argtypes = [_vp, _vp, _dp]
    if hasattr(L, "visma_icp_cloud_create"):             # (A/B runs load older builds through VISMA_ICP_LIB)
        _i64, _vp, _out = C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_void_p)
        L.visma_icp_cloud_create.argtypes = [_vp, _dp, C.c_int64, _dp, _dp, _out]
        L.visma_icp_cloud_from_tsdf.argtypes = [_vp, _vp, C.c_int, _out]
        L.visma_icp_cloud_destroy.argtypes = [_vp, _vp]
        L.visma_icp_cloud_size.argtypes = [_vp, _i64, C.POINTER(C.c_int)]
        L.visma_icp_cloud_get.argtypes = [_vp, _vp, _dp, _dp, _dp, C.c_int64]
        for name in ("transform", "paint_uniform_color", "orient_normals_to_align_with_direction",
                     "orient_normals_towards_camera_location", "mahalanobis_distance"):
            getattr(L, "visma_icp_cloud_" + name).argtypes = [_vp, _vp, _dp]
        L.visma_icp_cloud_normalize_normals.argtypes = [_vp, _vp]
        L.visma_icp_cloud_append.argtypes = [_vp, _vp, _vp]
        L.visma_icp_cloud_bounds.argtypes = [_vp, _vp, _dp, _dp]
        L.visma_icp_cloud_mean_and_covariance.argtypes = [_vp, _vp, _dp, _dp]
        L.visma_icp_cloud_select.argtypes = [_vp, _vp, _i64, C.c_int64, _out]
        L.visma_icp_cloud_uniform_down_sample.argtypes = [_vp, _vp, C.c_int64, _out]
        L.visma_icp_cloud_crop.argtypes = [_vp, _vp, _dp, _dp, _out]
        L.visma_icp_cloud_voxel_down_sample.argtypes = [_vp, _vp, C.c_double, _out]
        L.visma_icp_cloud_estimate_normals.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_double]
    if hasattr(L, "visma_icp_image_create"):             # (A/B runs load older builds through VISMA_ICP_LIB)
        _vp, _out, _ci, _cd = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_double
        L.visma_icp_image_create.argtypes = [_vp, _ci, _ci, _ci, _ci, _vp, _out]
        L.visma_icp_image_destroy.argtypes = [_vp, _vp]
        L.visma_icp_image_info.argtypes = [_vp] + [C.POINTER(_ci)] * 4
        L.visma_icp_image_get.argtypes = [_vp, _vp, _vp, C.c_int64]
        for name in ("copy", "flip", "downsample"):
            getattr(L, "visma_icp_image_" + name).argtypes = [_vp, _vp, _out]
        for name in ("to_float", "from_float", "filter", "dilate"):
            getattr(L, "visma_icp_image_" + name).argtypes = [_vp, _vp, _ci, _out]
        L.visma_icp_image_depth_to_float.argtypes = [_vp, _vp, _cd, _cd, _out]
        L.visma_icp_image_filter_separable.argtypes = [_vp, _vp, _dp, _ci, _dp, _ci, _out]
        L.visma_icp_image_filter_horizontal.argtypes = [_vp, _vp, _dp, _ci, _out]
        L.visma_icp_image_linear_transform.argtypes = [_vp, _vp, _cd, _cd]
        L.visma_icp_image_clip_intensity.argtypes = [_vp, _vp, _cd, _cd]
        L.visma_icp_image_pyramid.argtypes = [_vp, _vp, _ci, _ci, _out]
        L.visma_icp_image_filter_pyramid.argtypes = [_vp, _out, _ci, _ci, _out]
        L.visma_icp_image_distance_multiplier.argtypes = [_vp, _dp, _ci, _ci, _out]
        L.visma_icp_image_float_value_at.argtypes = [_vp, _vp, _dp, C.c_int64, C.POINTER(C.c_uint8), _dp]
        L.visma_icp_image_rgbd.argtypes = [_vp, _vp, _vp, _ci, _cd, _cd, _ci, _out, _out]
        L.visma_icp_tsdf_integrate_images.argtypes = [_vp, _vp, _vp, _vp, _dp, _ci, _ci, _dp]
        L.visma_icp_odometry_prepare_images.argtypes = [_vp, _vp, _vp, _vp, _vp, _dp, _dp, C.POINTER(COdometryOption)]
        L.visma_icp_rgbd_odometry_images.argtypes = [_vp, _vp, _vp, _vp, _vp, _dp, _dp, _ci, C.POINTER(COdometryOption), _dp, _dp,
                                                     C.POINTER(COdometryResult)]
        L.visma_icp_image_from_odometry.argtypes = [_vp, _ci, _ci, _out]
        L.visma_icp_cloud_from_depth_image.argtypes = [_vp, _vp, _dp, _dp, _cd, _cd, _ci, _out]
        L.visma_icp_cloud_from_rgbd_images.argtypes = [_vp, _vp, _vp, _dp, _dp, _out]
    if hasattr(L, "visma_icp_render"):                   # (A/B runs load older builds through VISMA_ICP_LIB)
        _vp, _out, _ci, _cd, _u8 = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_double, C.POINTER(C.c_uint8)
        L.visma_icp_render.argtypes = [_vp, _vp, _ci, _ci, _dp, _dp, _cd, _cd, _ci, _out, _out, _out]
        L.visma_icp_render_edges.argtypes = [_vp, _vp, _out]
        L.visma_icp_render_host.argtypes = [_dp, C.c_int64, _ip, C.c_int64, _ci, _ci, _dp, _dp, _cd, _cd, _ci, _fp, _ip, _u8, _u8]
        L.visma_icp_render_edges_host.argtypes = [_fp, _ci, _ci, _u8]
        L.visma_icp_linearize_depth.argtypes = [_cd, _cd, _cd]
        L.visma_icp_linearize_depth.restype = _cd
        L.visma_icp_image_is_int32.argtypes = [_vp, C.POINTER(_ci)]
    if hasattr(L, "visma_icp_color_map_create"):         # (A/B runs load older builds through VISMA_ICP_LIB)
        _i64, _vp, _u8 = C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_uint8)
        _opt = C.POINTER(CColorMapOption)
        L.visma_icp_color_map_option_default.argtypes = [_opt]
        L.visma_icp_color_map_option_default.restype = None
        L.visma_icp_color_map_create.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _dp, _opt, C.POINTER(_vp)]
        L.visma_icp_color_map_destroy.argtypes = [_vp, _vp]
        L.visma_icp_color_map_set_image.argtypes = [_vp, _vp, C.c_int, _fp, _u8, C.c_int, _dp]
        L.visma_icp_color_map_set_vertices.argtypes = [_vp, _vp, _dp, C.c_int64]
        L.visma_icp_color_map_prepare.argtypes = [_vp, _vp, _i64]
        L.visma_icp_color_map_get_image.argtypes = [_vp, _vp, C.c_int, C.c_int, _vp]
        L.visma_icp_color_map_get_visible.argtypes = [_vp, _vp, C.c_int, _ip, C.c_int64, _i64]
        L.visma_icp_color_map_get_proxy.argtypes = [_vp, _vp, _dp, C.c_int64]
        L.visma_icp_color_map_sums.argtypes = [_vp, _vp, _dp]
        L.visma_icp_color_map_step.argtypes = [_vp, _vp, _dp, _i64]
        L.visma_icp_color_map_run.argtypes = [_vp, _vp, C.c_int, _dp]
        L.visma_icp_color_map_get_extrinsics.argtypes = [_vp, _vp, _dp]
        L.visma_icp_color_map_set_extrinsics.argtypes = [_vp, _vp, _dp]
        L.visma_icp_color_map_get_colors.argtypes = [_vp, _vp, _dp, C.c_int64]
        L.visma_icp_color_map_optimization.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _dp, _fp, _u8, _dp, _dp, C.c_int64, _opt, _dp]
    if hasattr(L, "visma_icp_color_map_create_non_rigid"):
        _i64, _vp, _u8 = C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_uint8)
        _opt = C.POINTER(CColorMapOption)
        L.visma_icp_color_map_create_non_rigid.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _dp, _opt, C.POINTER(_vp)]
        L.visma_icp_color_map_get_anchor_shape.argtypes = [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.visma_icp_color_map_get_flow.argtypes = [_vp, _vp, _dp]
        L.visma_icp_color_map_set_flow.argtypes = [_vp, _vp, _dp]
        L.visma_icp_color_map_cell_sums.argtypes = [_vp, _vp, _dp]
        L.visma_icp_color_map_step_non_rigid.argtypes = [_vp, _vp, _dp, _dp, _i64]
        L.visma_icp_color_map_optimization_non_rigid.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _dp, _fp, _u8, _dp, _dp, C.c_int64, _opt, _dp, _dp]
        L.visma_icp_color_map_solve_non_rigid.argtypes = [C.c_int, C.c_int, _dp, C.c_int64, C.c_double, _dp, _dp, _dp,
                                                          C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.visma_icp_set_persistent_cu_share.argtypes = [C.c_double]
    L.visma_icp_get_persistent_info.argtypes = [C.c_void_p, C.POINTER(CPersistentInfo)]
    L.visma_icp_get_timing_sized.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.visma_icp_get_timing.argtypes = [C.c_void_p, C.POINTER(CTiming), C.c_int]
    L.visma_icp_get_tile_config.argtypes = [C.POINTER(C.c_int)] * 3
    L.visma_icp_get_launch_config.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.visma_icp_comm_unique_id.argtypes = [C.c_void_p]
    L.visma_icp_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.visma_icp_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p, C.c_int, C.c_int]
    L.visma_so3_rodrigues.argtypes = [_dp, _dp, _dp]
    L.visma_so3_invrodrigues.argtypes = [_dp, _dp, _dp]
    L.visma_so3_project.argtypes = [_dp, _dp]
    L.visma_so3_matrix_derivatives.argtypes = [_dp] * 7
    L.visma_icp_selftest_so3_jac.argtypes = [_dp, C.c_int, _dp, _dp, _dp, _dp, _dp]
    L.visma_icp_selftest_neighbor_lists.argtypes = [_dp, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int,
                                                    C.POINTER(C.c_int32), _dp, C.POINTER(C.c_int32)]
    L.visma_icp_run_yaw_sweep_point_to_plane.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double,
                                                         C.c_double, C.POINTER(CResult), C.POINTER(C.c_int),
                                                         C.POINTER(CResult)]
    L.visma_icp_comm_ipc_export.argtypes = [C.c_void_p, C.c_void_p]
    L.visma_icp_comm_ipc_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.visma_icp_set_global_source_count.argtypes = [C.c_void_p, C.c_int64]
    return L


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def _p(a, t):
    return a.ctypes.data_as(t)


class CTrimInfo(C.Structure):
    """visma_icp_trim_info"""
    _fields_ = [("kept", C.c_int64), ("trimmed_rmse", C.c_double), ("d2_cut", C.c_double)]


class TrimInfo:
    """What a trimmed pass kept: m pairs, their rmse, the largest kept fp32 squared distance."""

    def __init__(self, c):
        self.kept = int(c.kept)
        self.trimmed_rmse = float(c.trimmed_rmse)
        self.d2_cut = float(c.d2_cut)

    def __repr__(self):
        return "TrimInfo(kept=%d, trimmed_rmse=%.6g, d2_cut=%.6g)" % (self.kept, self.trimmed_rmse, self.d2_cut)


ROBUST_L2, ROBUST_HUBER, ROBUST_TUKEY, ROBUST_CAUCHY = 0, 1, 2, 3
_ROBUST_NAMES = {"l2": ROBUST_L2, "huber": ROBUST_HUBER, "tukey": ROBUST_TUKEY, "cauchy": ROBUST_CAUCHY}


class CRobust(C.Structure):
    """visma_icp_robust"""
    _fields_ = [("kernel", C.c_int), ("scale", C.c_double), ("tune", C.c_double), ("min_scale", C.c_double)]


class CRobustInfo(C.Structure):
    """visma_icp_robust_info"""
    _fields_ = [("scale", C.c_double), ("median_residual", C.c_double), ("weight_sum", C.c_double),
                ("zero_weight", C.c_int64), ("robust_rmse", C.c_double)]


def _robust(kernel, scale, tune, min_scale):
    if isinstance(kernel, str):
        kernel = _ROBUST_NAMES[kernel.lower()]
    return CRobust(int(kernel), float(scale), float(tune), float(min_scale))


class RobustInfo:
    """What the weights of a robust pass did: the scale c, the median residual it came from (automatic scale), the sum
    of the weights, the pairs with weight 0 and the weighted rmse."""

    def __init__(self, c):
        self.scale = float(c.scale)
        self.median_residual = float(c.median_residual)
        self.weight_sum = float(c.weight_sum)
        self.zero_weight = int(c.zero_weight)
        self.robust_rmse = float(c.robust_rmse)

    def __repr__(self):
        return "RobustInfo(scale=%.6g, median_residual=%.6g, weight_sum=%.6g, zero_weight=%d, robust_rmse=%.6g)" % (
            self.scale, self.median_residual, self.weight_sum, self.zero_weight, self.robust_rmse)


class CGicpInfo(C.Structure):
    """visma_icp_gicp_info"""
    _fields_ = [("cost", C.c_double), ("mahalanobis_rmse", C.c_double)]


class GicpInfo:
    """A generalized pass: cost = sum d^T M d over its pairs and mahalanobis_rmse = sqrt(cost / K)."""

    def __init__(self, c):
        self.cost = float(c.cost)
        self.mahalanobis_rmse = float(c.mahalanobis_rmse)

    def __repr__(self):
        return "GicpInfo(cost=%.6g, mahalanobis_rmse=%.6g)" % (self.cost, self.mahalanobis_rmse)


class CColoredInfo(C.Structure):
    """visma_icp_colored_info"""
    _fields_ = [("cost", C.c_double), ("geometric_cost", C.c_double), ("photometric_cost", C.c_double)]


class ColoredInfo:
    """A colored pass: cost = sum r_g^2 + r_c^2 over its pairs (the reference's ComputeRMSE) and its two parts."""

    def __init__(self, c):
        self.cost = float(c.cost)
        self.geometric_cost = float(c.geometric_cost)
        self.photometric_cost = float(c.photometric_cost)

    def __repr__(self):
        return "ColoredInfo(cost=%.6g, geometric_cost=%.6g, photometric_cost=%.6g)" % (
            self.cost, self.geometric_cost, self.photometric_cost)


class CFgrOption(C.Structure):
    """visma_icp_fgr_option (defaults: FastGlobalRegistration.h:44-50)"""
    _fields_ = [("division_factor", C.c_double), ("max_corr_dist", C.c_double), ("tuple_scale", C.c_double),
                ("use_absolute_scale", C.c_int), ("decrease_mu", C.c_int), ("iteration_number", C.c_int),
                ("maximum_tuple_count", C.c_int)]


class CFgrInfo(C.Structure):
    """visma_icp_fgr_info"""
    _fields_ = [("n_mutual", C.c_int64), ("n_tuple_corres", C.c_int64), ("n_trials", C.c_int64)]


FPFH_DIM = 33


def fgr_option(division_factor=1.4, max_corr_dist=0.025, tuple_scale=0.95, use_absolute_scale=False, decrease_mu=True,
               iteration_number=64, maximum_tuple_count=1000):
    return CFgrOption(float(division_factor), float(max_corr_dist), float(tuple_scale), int(bool(use_absolute_scale)),
                      int(bool(decrease_mu)), int(iteration_number), int(maximum_tuple_count))


class FgrInfo:
    """What fast global registration's matching did: pairs after the cross check, pairs the tuple test pushed, trials drawn."""

    def __init__(self, c):
        self.n_mutual = int(c.n_mutual)
        self.n_tuple_corres = int(c.n_tuple_corres)
        self.n_trials = int(c.n_trials)

    def __repr__(self):
        return "FgrInfo(n_mutual=%d, n_tuple_corres=%d, n_trials=%d)" % (self.n_mutual, self.n_tuple_corres, self.n_trials)


def _fgr_triples(triples):
    if triples is None:
        return None, 0, None
    t = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    return t, len(t), _p(t, _ip)


def fgr_optimize(src, tgt, src_idx, tgt_idx, option=None):
    """Fast global registration's optimisation over given pairs (host only) -> (T source-to-target, the normalized-frame
    result of OptimizePairwiseRegistration)."""
    s = _f64(src, (-1, 3)); t = _f64(tgt, (-1, 3))
    si = np.ascontiguousarray(src_idx, np.int32).ravel(); ti = np.ascontiguousarray(tgt_idx, np.int32).ravel()
    if len(si) != len(ti):
        raise ValueError("fgr_optimize: one target index per source index")
    T = np.empty(16); Topt = np.empty(16)
    o = option if option is not None else fgr_option()
    rc = load().visma_icp_fgr_optimize(_p(s, _dp), len(s), _p(t, _dp), len(t), _p(si, _ip), _p(ti, _ip), len(si), C.byref(o),
                                       _p(T, _dp), _p(Topt, _dp))
    if rc != OK:
        raise IcpError(rc, "fgr_optimize: bad arguments")
    return T.reshape(4, 4), Topt.reshape(4, 4)


class CRansacOption(C.Structure):
    """visma_icp_ransac_option (defaults: Registration.h:61-78, every checker off)"""
    _fields_ = [("ransac_n", C.c_int), ("max_iteration", C.c_int), ("max_validation", C.c_int),
                ("edge_length_similarity", C.c_double), ("distance_threshold", C.c_double), ("normal_angle", C.c_double),
                ("chunk_trials", C.c_int)]


class CRansacInfo(C.Structure):
    """visma_icp_ransac_info"""
    _fields_ = [("n_trials", C.c_int64), ("n_rejected_before", C.c_int64), ("n_rejected_after", C.c_int64),
                ("n_validated", C.c_int64), ("best_trial", C.c_int64), ("hypothesis_ms", C.c_double), ("validation_ms", C.c_double)]


RANSAC_PASS, RANSAC_REJECTED_BEFORE, RANSAC_REJECTED_AFTER = 0, 1, 2


def ransac_option(ransac_n=4, max_iteration=1000, max_validation=1000, edge_length_similarity=0.0, distance_threshold=0.0,
                  normal_angle=0.0, chunk_trials=0):
    """A checker threshold <= 0 turns that checker off; chunk_trials 0: the library's choice."""
    return CRansacOption(int(ransac_n), int(max_iteration), int(max_validation), float(edge_length_similarity),
                         float(distance_threshold), float(normal_angle), int(chunk_trials))


class RansacInfo:
    """What the RANSAC loop did: trials consumed, rejected before / after alignment, validated, the best trial (-1: none)."""

    def __init__(self, c):
        self.n_trials = int(c.n_trials)
        self.n_rejected_before = int(c.n_rejected_before)
        self.n_rejected_after = int(c.n_rejected_after)
        self.n_validated = int(c.n_validated)
        self.best_trial = int(c.best_trial)
        self.hypothesis_ms = float(c.hypothesis_ms)
        self.validation_ms = float(c.validation_ms)

    def __repr__(self):
        return ("RansacInfo(n_trials=%d, n_rejected_before=%d, n_rejected_after=%d, n_validated=%d, best_trial=%d)"
                % (self.n_trials, self.n_rejected_before, self.n_rejected_after, self.n_validated, self.best_trial))


def _ransac_draws(draws, ransac_n):
    if draws is None:
        return None, 0, None
    d = np.ascontiguousarray(draws, np.int32).reshape(-1, max(int(ransac_n), 1))
    return d, len(d), _p(d, _ip)


def _ransac_hyp_args(src, tgt, src_normals, tgt_normals, pair_src, pair_tgt, option, draws, first_trial, n_trials):
    s = _f64(src, (-1, 3)); t = _f64(tgt, (-1, 3))
    sn = None if src_normals is None else _f64(src_normals, (-1, 3))
    tn = None if tgt_normals is None else _f64(tgt_normals, (-1, 3))
    ps = None if pair_src is None else np.ascontiguousarray(pair_src, np.int32).ravel()
    pt = np.ascontiguousarray(pair_tgt, np.int32).ravel()
    if (sn is not None and len(sn) != len(s)) or (tn is not None and len(tn) != len(t)) or (ps is not None and len(ps) != len(pt)):
        raise ValueError("ransac_hypotheses: one normal per point, one target index per source index")
    o = option if option is not None else ransac_option()
    d, nd, dp_ = _ransac_draws(draws, o.ransac_n)
    if d is not None and nd < int(first_trial) + int(n_trials):
        raise ValueError("ransac_hypotheses: draws for every trial from 0")
    verdict = np.zeros(max(int(n_trials), 1), np.int8); T = np.zeros((max(int(n_trials), 1), 16))
    keep = (s, t, sn, tn, ps, pt, d)
    return keep, o, verdict, T, [_p(s, _dp), len(s), _p(t, _dp), len(t), None if sn is None else _p(sn, _dp),
                                 None if tn is None else _p(tn, _dp), None if ps is None else _p(ps, _ip), _p(pt, _ip), len(pt),
                                 C.byref(o)]


def ransac_hypotheses_host(src, tgt, pair_tgt, option=None, seed=0, draws=None, first_trial=0, n_trials=0, src_normals=None,
                           tgt_normals=None, pair_src=None):
    """The hypothesis stage of RANSAC on the host (no context): the functions the kernels run
    -> (verdict (n,) int8, T (n, 4, 4))."""
    keep, o, verdict, T, args = _ransac_hyp_args(src, tgt, src_normals, tgt_normals, pair_src, pair_tgt, option, draws, first_trial,
                                                 n_trials)
    rc = load().visma_icp_ransac_hypotheses_host(*args, int(seed), None if keep[6] is None else _p(keep[6], _ip), int(first_trial),
                                                 int(n_trials), _p(verdict, C.POINTER(C.c_int8)), _p(T, _dp))
    if rc != OK:
        raise IcpError(rc, "ransac_hypotheses_host: bad arguments")
    return verdict[:int(n_trials)].copy(), T[:int(n_trials)].reshape(-1, 4, 4).copy()


def render_host(vertices, triangles, w, h, intrinsic, extrinsic=None, z_near=0.05, z_far=10.0, encoding="metric"):
    """TriMesh.render and Context.render_edges on the host: the same arithmetic, no context, no GPU -> depth (h x w float32),
    index (int32), mask (uint8), edges (uint8; of the metric depth whatever the encoding).  Bad arguments: IcpError, nothing
    computed."""
    v = _f64(vertices, (-1, 3))
    t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    k = _f64(intrinsic, (4,)); E = _f64(np.eye(4) if extrinsic is None else extrinsic, (16,))
    w, h = int(w), int(h)
    shape = (max(h, 0), max(w, 0))
    depth, index = np.zeros(shape, np.float32), np.zeros(shape, np.int32)
    mask, edges = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    u8 = C.POINTER(C.c_uint8)
    rc = load().visma_icp_render_host(_p(v, _dp), len(v), _p(t, _ip), len(t), w, h, _p(k, _dp), _p(E, _dp), float(z_near), float(z_far),
                                      _image_enum(encoding, RENDER_ENCODINGS), _p(depth, _fp), _p(index, _ip), _p(mask, u8), _p(edges, u8))
    if rc != OK:
        raise IcpError(rc, "render_host: bad arguments")
    return depth, index, mask, edges


def render_edges_host(depth):
    """Context.render_edges on a host array (h x w float32, metric) -> h x w uint8"""
    d = np.ascontiguousarray(depth, dtype=np.float32)
    out = np.zeros(d.shape, np.uint8)
    if d.ndim != 2:
        raise ValueError("an h x w array")
    rc = load().visma_icp_render_edges_host(_p(d, _fp), d.shape[1], d.shape[0], _p(out, C.POINTER(C.c_uint8)))
    if rc != OK:
        raise IcpError(rc, "render_edges_host: bad arguments")
    return out


def linearize_depth(zb, z_near, z_far):
    """LinearizeDepth (renderer.h): the metric depth of a depth-buffer value, in f64"""
    return load().visma_icp_linearize_depth(float(zb), float(z_near), float(z_far))


class PoseGraphEdge:
    """An edge of a pose graph (Open3D's PoseGraphEdge): `transformation` maps the source node's cloud onto the target
    node's; loop closures are `uncertain`; `confidence` is the line-process value."""

    def __init__(self, source, target, transformation=None, information=None, uncertain=False, confidence=1.0):
        self.source = int(source); self.target = int(target)
        self.transformation = _f64(np.eye(4) if transformation is None else transformation, (4, 4)).copy()
        self.information = _f64(np.eye(6) if information is None else information, (6, 6)).copy()
        self.uncertain = bool(uncertain)
        self.confidence = float(confidence)

    def __repr__(self):
        return "PoseGraphEdge(%d -> %d, uncertain=%s, confidence=%.6g)" % (self.source, self.target, self.uncertain, self.confidence)


def global_optimization_option(max_correspondence_distance=0.075, edge_prune_threshold=0.25, preference_loop_closure=1.0,
                               reference_node=-1):
    """GlobalOptimizationOption, clamped as the reference's constructor clamps."""
    o = CGlobalOptimizationOption(float(max_correspondence_distance), float(edge_prune_threshold), float(preference_loop_closure),
                                  int(reference_node))
    load().visma_icp_global_optimization_option_clamp(C.byref(o))
    return o


def global_optimization_criteria(max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                                 min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2. / 3.,
                                 lower_scale_factor=1. / 3.):
    """GlobalOptimizationConvergenceCriteria, clamped as the reference's constructor clamps."""
    c = CGlobalOptimizationCriteria(int(max_iteration), float(min_relative_increment), float(min_relative_residual_increment),
                                    float(min_right_term), float(min_residual), int(max_iteration_lm), float(upper_scale_factor),
                                    float(lower_scale_factor))
    load().visma_icp_global_optimization_criteria_clamp(C.byref(c))
    return c


def _pose_graph_args(poses, edges):
    P = _f64(poses, (-1, 16)).copy()
    arr = (CPoseGraphEdge * max(len(edges), 1))()
    for i, e in enumerate(edges):
        arr[i].source = e.source; arr[i].target = e.target
        arr[i].transformation = (C.c_double * 16)(*_f64(e.transformation, (16,)))
        arr[i].information = (C.c_double * 36)(*_f64(e.information, (36,)))
        arr[i].uncertain = 1 if e.uncertain else 0
        arr[i].confidence = float(e.confidence)
    return P, arr


def marching_cubes_case(cube_case):
    """The triangles of one case of ExtractTriangleMesh's case rule as edge ids (t x 3 int32, t <= 5); host only.
    Bit i of cube_case: the corner at offset (i & 1, (i >> 1) & 1, (i >> 2) & 1) is inside; edge id 4 axis + j."""
    ids = np.zeros(15, np.int32)
    n = C.c_int(0)
    rc = load().visma_icp_marching_cubes_case(int(cube_case), _p(ids, _ip), C.byref(n))
    if rc:
        raise IcpError(rc, "marching_cubes_case: a case outside 0 .. 255")
    return ids[:3 * n.value].reshape(-1, 3).copy()


def pose_graph_validate(n_nodes, edges):
    """ValidatePoseGraph: every consecutive node pair has an edge and every edge names nodes of the graph."""
    _, arr = _pose_graph_args(np.zeros((0, 16)), edges)
    rc = load().visma_icp_pose_graph_validate(int(n_nodes), arr, len(edges))
    if rc < 0 or rc > 1:
        raise IcpError(rc, "pose_graph_validate: bad arguments")
    return bool(rc)


def pose_graph_zeta(poses, edges):
    """The linearised misalignment of every edge at the given poses (n x 4 x 4) -> n_edges x 6 (host only)."""
    P, arr = _pose_graph_args(poses, edges)
    z = np.zeros((max(len(edges), 1), 6))
    rc = load().visma_icp_pose_graph_zeta(_p(P, _dp), len(P), arr, len(edges), _p(z, _dp))
    if rc != OK:
        raise IcpError(rc, "pose_graph_zeta: bad arguments")
    return z[:len(edges)]


def pose_graph_linear_system(poses, edges):
    """H (6n x 6n) and b (6n) of the Gauss-Newton step at the given poses with the edges' confidences (host only)."""
    P, arr = _pose_graph_args(poses, edges)
    n = 6 * len(P)
    H = np.zeros((max(n, 1), max(n, 1))); b = np.zeros(max(n, 1))
    rc = load().visma_icp_pose_graph_linear_system(_p(P, _dp), len(P), arr, len(edges), _p(H, _dp), _p(b, _dp))
    if rc != OK:
        raise IcpError(rc, "pose_graph_linear_system: bad arguments")
    return (H[:n, :n], b[:n]) if n else (np.zeros((0, 0)), np.zeros(0))


_GLOBAL_METHODS = {"gn": 0, "gauss_newton": 0, "gauss-newton": 0, "lm": 1, "levenberg_marquardt": 1, "levenberg-marquardt": 1}


def pose_graph_optimize(poses, edges, method="lm", criteria=None, option=None):
    """ONE optimisation of a pose graph (GlobalOptimizationMethod::OptimizePoseGraph; host only): no validation, no pruning,
    no compensation of the reference node -> (poses, the edges with their new confidences)."""
    m = _GLOBAL_METHODS.get(method.lower()) if isinstance(method, str) else int(method)
    if m not in (0, 1):
        raise ValueError("pose_graph_optimize: method is 'gn' or 'lm'")
    P, arr = _pose_graph_args(poses, edges)
    rc = load().visma_icp_pose_graph_optimize(_p(P, _dp), len(P), arr, len(edges), m,
                                              C.byref(criteria) if criteria is not None else None,
                                              C.byref(option) if option is not None else None)
    if rc != OK:
        raise IcpError(rc, "pose_graph_optimize: bad arguments")
    out = [PoseGraphEdge(arr[i].source, arr[i].target, np.array(arr[i].transformation[:]), np.array(arr[i].information[:]),
                         arr[i].uncertain != 0, arr[i].confidence) for i in range(len(edges))]
    return P.reshape(-1, 4, 4), out


def global_optimization(poses, edges, method="lm", criteria=None, option=None):
    """Open3D's GlobalOptimization on a pose graph (host only): poses n x 4 x 4, edges PoseGraphEdge objects ->
    (poses, the edges that survive the pruning with their confidences).  An invalid graph (pose_graph_validate) comes
    back unchanged."""
    m = _GLOBAL_METHODS.get(method.lower()) if isinstance(method, str) else int(method)
    if m not in (0, 1):
        raise ValueError("global_optimization: method is 'gn' or 'lm'")
    P, arr = _pose_graph_args(poses, edges)
    ne = C.c_int(len(edges))
    rc = load().visma_icp_global_optimization(_p(P, _dp), len(P), arr, C.byref(ne), m,
                                              C.byref(criteria) if criteria is not None else None,
                                              C.byref(option) if option is not None else None)
    if rc != OK:
        raise IcpError(rc, "global_optimization: bad arguments")
    out = [PoseGraphEdge(arr[i].source, arr[i].target, np.array(arr[i].transformation[:]), np.array(arr[i].information[:]),
                         arr[i].uncertain != 0, arr[i].confidence) for i in range(ne.value)]
    return P.reshape(-1, 4, 4), out


class Result:
    """Mirror of open3d::RegistrationResult (+ iteration counts)."""

    def __init__(self, c):
        self.transformation_ = np.array(list(c.transformation), dtype=np.float64).reshape(4, 4)
        self.fitness_ = float(c.fitness)
        self.inlier_rmse_ = float(c.inlier_rmse)
        self.num_correspondences = int(c.num_correspondences)
        self.iterations = int(c.iterations)
        self.nn_passes = int(c.nn_passes)
        self.correspondence_set_ = None

    def __repr__(self):
        return ("RegistrationResult(fitness=%.6f, inlier_rmse=%.6g, K=%d, iterations=%d)" %
                (self.fitness_, self.inlier_rmse_, self.num_correspondences, self.iterations))


class Context:
    """One ICP context = one HIP stream on one GPU (visma_icp_ctx)."""

    def __init__(self, device=0, engine=None):
        self.L = load() if engine is None else load_seams()
        self._h = C.c_void_p()
        self._keep = []
        if engine is None:
            rc = self.L.visma_icp_create(C.byref(self._h), int(device))
        else:
            self._keep.append(engine)
            rc = self.L.visma_icp_create_with_engine(C.byref(self._h), C.byref(engine), None)
        if rc != OK:
            msg = self.L.visma_icp_last_error(None)
            raise IcpError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.L.visma_icp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            msg = self.L.visma_icp_last_error(self._h)
            raise IcpError(rc, msg.decode() if msg else "")

    # ---- clouds ----
    def set_clouds_f64(self, src, tgt):
        src = _f64(src, (-1, 3)); tgt = _f64(tgt, (-1, 3))
        self._chk(self.L.visma_icp_set_clouds_f64(self._h, _p(src, _dp), len(src), 3,
                                                  _p(tgt, _dp), len(tgt), 3))
        self.ns, self.nt = len(src), len(tgt)

    def set_clouds_f64_voxel_target(self, src, scene, voxel_size):
        """target = VoxelDownSample(scene, voxel_size), made and installed on the device -> its point count."""
        s = _f64(src, (-1, 3)); t = _f64(scene, (-1, 3))
        nt = C.c_int64(0)
        self._chk(self.L.visma_icp_set_clouds_f64_voxel_target(self._h, _p(s, _dp), len(s), 3, _p(t, _dp), len(t), 3,
                                                               float(voxel_size), C.byref(nt)))
        self.ns, self.nt = len(s), int(nt.value)
        return int(nt.value)

    def set_clouds_meshes_f64(self, meshes, scene, voxel_size=0.0, reference_quirks=0, seed=0):
        """meshes: [(V (nv,3) f64, F (nf,3) i32, samples, T (4,4) or None)]; the source is sampled, moved and
        concatenated on the device (feh::ICPRefinement's scene_est), the scene optionally voxel-down-sampled there.
        Returns (ns, nt)."""
        keep = []
        arr = (CMeshSource * max(len(meshes), 1))()
        for k, (V, F, n, T) in enumerate(meshes):
            V = np.ascontiguousarray(V, np.float64); F = np.ascontiguousarray(F, np.int32)
            Tm = None if T is None else np.ascontiguousarray(T, np.float64).reshape(16)
            keep += [V, F, Tm]
            arr[k].V = _p(V, _dp); arr[k].nv = len(V)
            arr[k].F = _p(F, C.POINTER(C.c_int32)); arr[k].nf = len(F)
            arr[k].samples = int(n)
            arr[k].model_to_scene = _p(Tm, _dp) if Tm is not None else None
        scene = np.ascontiguousarray(scene, np.float64)
        ns, nt = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.visma_icp_set_clouds_meshes_f64(self._h, arr, len(meshes), int(reference_quirks), int(seed),
                                                         _p(scene, _dp), len(scene), 3, float(voxel_size),
                                                         C.byref(ns), C.byref(nt)))
        self.ns, self.nt = int(ns.value), int(nt.value)
        return self.ns, self.nt

    def set_radius_hint(self, r):
        """The search radius of the next registration: the next upload builds the grid while it stages the source."""
        self._chk(self.L.visma_icp_set_radius_hint(self._h, float(r)))

    def get_mesh_source(self, ns):
        out = np.empty((int(ns), 3), np.float64)
        self._chk(self.L.visma_icp_get_mesh_source(self._h, _p(out, _dp), int(ns)))
        return out

    def get_voxel_target(self, nt):
        out = np.empty((max(nt, 1), 3))
        self._chk(self.L.visma_icp_get_voxel_target(self._h, _p(out, _dp), int(nt)))
        return out[:nt].copy()

    def set_target(self, xyz):
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        self._chk(self.L.visma_icp_set_target(self._h, _p(a, _fp), a.shape[0], a.shape[1]))
        self.nt = a.shape[0]

    def set_source(self, xyz):
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        self._chk(self.L.visma_icp_set_source(self._h, _p(a, _fp), a.shape[0], a.shape[1]))
        self.ns = a.shape[0]

    def set_target_device(self, ptr, n):
        self._chk(self.L.visma_icp_set_target_device(self._h, C.c_void_p(ptr), n))
        self.nt = n

    def set_source_device(self, ptr, n):
        self._chk(self.L.visma_icp_set_source_device(self._h, C.c_void_p(ptr), n))
        self.ns = n

    def set_target_normals_f64(self, n):
        n = _f64(n, (-1, 3))
        self._chk(self.L.visma_icp_set_target_normals_f64(self._h, _p(n, _dp), len(n), 3))

    # ---- kernels ----
    def nn_pass(self, T, max_dist):
        T = _f64(T, (16,))
        self._chk(self.L.visma_icp_nn_pass(self._h, _p(T, _dp), float(max_dist)))

    def reduce(self):
        st = np.empty(NSTATS)
        self._chk(self.L.visma_icp_reduce(self._h, _p(st, _dp)))
        return st

    def reduce_trimmed(self, keep):
        """The statistics of the last nn_pass over the floor(keep * ns) pairs with the smallest (d2, source index)
        -> (stats, TrimInfo)."""
        st = np.empty(NSTATS); info = CTrimInfo()
        self._chk(self.L.visma_icp_reduce_trimmed(self._h, float(keep), _p(st, _dp), C.byref(info)))
        return st, TrimInfo(info)

    def kept_mask(self):
        """bool per source point (caller's order): kept by the last trimmed pass."""
        m = np.zeros(max(self.ns, 1), np.uint8)
        self._chk(self.L.visma_icp_get_kept_mask(self._h, _p(m, C.POINTER(C.c_uint8))))
        return m[:self.ns].astype(bool)

    def get_correspondences(self):
        si = np.empty(max(self.ns, 1), np.int32); ti = np.empty(max(self.ns, 1), np.int32)
        d2 = np.empty(max(self.ns, 1), np.float32); k = C.c_int64(0)
        self._chk(self.L.visma_icp_get_correspondences(self._h, _p(si, _ip), _p(ti, _ip),
                                                       _p(d2, _fp), C.byref(k)))
        k = k.value
        return si[:k].copy(), ti[:k].copy(), d2[:k].copy()

    def correspondence_index(self):
        """Per-source-point target index (-1 = none), like the oracle's idx."""
        si, ti, _ = self.get_correspondences()
        idx = np.full(self.ns, -1, np.int32)
        idx[si] = ti
        return idx

    # ---- loops ----
    def run(self, init=None, max_dist=0.05, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
            solver=SOLVER_KABSCH, with_scaling=False):
        init = _f64(np.eye(4) if init is None else init, (16,))
        out = CResult()
        self._chk(self.L.visma_icp_run(self._h, _p(init, _dp), float(max_dist), int(max_iter),
                                       float(rel_fitness), float(rel_rmse), int(solver),
                                       int(bool(with_scaling)), C.byref(out)))
        return Result(out)

    def run_trimmed(self, init=None, max_dist=0.05, keep=1.0, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                    solver=SOLVER_KABSCH, with_scaling=False):
        """Trimmed ICP: per pass only the floor(keep * ns) closest pairs enter the solve.  keep = the share of the
        source the target can see; a keep below the true overlap stalls.  -> Result with .trim (TrimInfo)."""
        init = _f64(np.eye(4) if init is None else init, (16,))
        out = CResult(); info = CTrimInfo()
        self._chk(self.L.visma_icp_run_trimmed(self._h, _p(init, _dp), float(max_dist), float(keep), int(max_iter),
                                               float(rel_fitness), float(rel_rmse), int(solver),
                                               int(bool(with_scaling)), C.byref(out), C.byref(info)))
        r = Result(out)
        r.trim = TrimInfo(info)
        return r

    def run_yaw_sweep_trimmed(self, level, max_dist, keep, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                              solver=SOLVER_KABSCH):
        best = CResult(); bl = C.c_int(-1); per = (CResult * level)()
        bi = CTrimInfo(); pi = (CTrimInfo * level)()
        self._chk(self.L.visma_icp_run_yaw_sweep_trimmed(self._h, int(level), float(max_dist), float(keep), int(max_iter),
                                                         float(rel_fitness), float(rel_rmse), int(solver), C.byref(best),
                                                         C.byref(bl), per, C.byref(bi), pi))
        rb = Result(best); rb.trim = TrimInfo(bi)
        rs = []
        for p, i in zip(per, pi):
            r = Result(p); r.trim = TrimInfo(i); rs.append(r)
        return rb, bl.value, rs

    def reduce_robust(self, kernel, scale=0.0, tune=0.0, min_scale=0.0, plane=False):
        """The statistics of the last nn_pass with every pair weighted by its residual (kernel: ROBUST_* or "huber",
        "tukey", "cauchy", "l2"; scale 0: from the median residual) -> (stats, RobustInfo)."""
        st = np.empty(NSTATS); info = CRobustInfo(); cfg = _robust(kernel, scale, tune, min_scale)
        self._chk(self.L.visma_icp_reduce_robust(self._h, C.byref(cfg), int(bool(plane)), _p(st, _dp), C.byref(info)))
        return st, RobustInfo(info)

    def pair_weights(self):
        """float64 per source point (caller's order): its weight in the last robust pass, 0 without a pair."""
        w = np.zeros(max(self.ns, 1))
        self._chk(self.L.visma_icp_get_pair_weights(self._h, _p(w, _dp)))
        return w[:self.ns]

    def run_robust(self, init=None, max_dist=0.05, kernel=ROBUST_TUKEY, scale=0.0, tune=0.0, min_scale=0.0, plane=False,
                   max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, with_scaling=False):
        """Robust ICP: every pair weighted by a function of its own residual; no overlap share is needed.
        -> Result with .robust (RobustInfo)."""
        init = _f64(np.eye(4) if init is None else init, (16,))
        out = CResult(); info = CRobustInfo(); cfg = _robust(kernel, scale, tune, min_scale)
        self._chk(self.L.visma_icp_run_robust(self._h, _p(init, _dp), float(max_dist), C.byref(cfg), int(bool(plane)),
                                              int(max_iter), float(rel_fitness), float(rel_rmse), int(bool(with_scaling)),
                                              C.byref(out), C.byref(info)))
        r = Result(out)
        r.robust = RobustInfo(info)
        return r

    def run_yaw_sweep_robust(self, level, max_dist, kernel=ROBUST_TUKEY, scale=0.0, tune=0.0, min_scale=0.0, plane=False,
                             max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        best = CResult(); bl = C.c_int(-1); per = (CResult * level)()
        bi = CRobustInfo(); pi = (CRobustInfo * level)(); cfg = _robust(kernel, scale, tune, min_scale)
        self._chk(self.L.visma_icp_run_yaw_sweep_robust(self._h, int(level), float(max_dist), C.byref(cfg), int(bool(plane)),
                                                        int(max_iter), float(rel_fitness), float(rel_rmse), C.byref(best),
                                                        C.byref(bl), per, C.byref(bi), pi))
        rb = Result(best); rb.robust = RobustInfo(bi)
        rs = []
        for p, i in zip(per, pi):
            r = Result(p); r.robust = RobustInfo(i); rs.append(r)
        return rb, bl.value, rs

    def set_source_normals_f64(self, n):
        """Normals of the source (caller's order, after the source is set; used as given): what generalized ICP needs
        next to the target's."""
        n = _f64(n, (-1, 3))
        self._chk(self.L.visma_icp_set_source_normals_f64(self._h, _p(n, _dp), len(n), 3))

    def reduce_gicp(self, epsilon=1e-3):
        """The generalized (plane-to-plane) statistics of the last nn_pass -> (stats, GicpInfo)."""
        st = np.empty(NSTATS); info = CGicpInfo()
        self._chk(self.L.visma_icp_reduce_gicp(self._h, float(epsilon), _p(st, _dp), C.byref(info)))
        return st, GicpInfo(info)

    def run_gicp(self, init=None, max_dist=0.05, epsilon=1e-3, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        """Generalized ICP: every pair weighted by the inverse of the sum of both points' surface covariances
        C = I - (1 - epsilon) n n^T; needs source and target normals.  -> Result with .gicp (GicpInfo)."""
        init = _f64(np.eye(4) if init is None else init, (16,))
        out = CResult(); info = CGicpInfo()
        self._chk(self.L.visma_icp_run_gicp(self._h, _p(init, _dp), float(max_dist), float(epsilon), int(max_iter),
                                            float(rel_fitness), float(rel_rmse), C.byref(out), C.byref(info)))
        r = Result(out)
        r.gicp = GicpInfo(info)
        return r

    def run_yaw_sweep_gicp(self, level, max_dist, epsilon=1e-3, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        best = CResult(); bl = C.c_int(-1); per = (CResult * level)()
        bi = CGicpInfo(); pi = (CGicpInfo * level)()
        self._chk(self.L.visma_icp_run_yaw_sweep_gicp(self._h, int(level), float(max_dist), float(epsilon), int(max_iter),
                                                      float(rel_fitness), float(rel_rmse), C.byref(best), C.byref(bl), per,
                                                      C.byref(bi), pi))
        rb = Result(best); rb.gicp = GicpInfo(bi)
        rs = []
        for p, i in zip(per, pi):
            r = Result(p); r.gicp = GicpInfo(i); rs.append(r)
        return rb, bl.value, rs

    def set_source_colors_f64(self, rgb):
        """Colours of the source (caller's order, after the source is set): colored ICP keeps I = (r + g + b) / 3."""
        c = _f64(rgb, (-1, 3))
        self._chk(self.L.visma_icp_set_source_colors_f64(self._h, _p(c, _dp), len(c), 3))

    def set_target_colors_f64(self, rgb):
        c = _f64(rgb, (-1, 3))
        self._chk(self.L.visma_icp_set_target_colors_f64(self._h, _p(c, _dp), len(c), 3))

    def prepare_colored(self, radius, max_nn=30):
        """The colour gradient of the target (Hybrid search: radius, max_nn), kept on the device; needs target normals
        and target colours."""
        self._chk(self.L.visma_icp_prepare_colored(self._h, float(radius), int(max_nn)))

    def color_gradient_of_target(self):
        """The kept gradient, (nt, 3) in the caller's order."""
        nt = int(getattr(self, "nt", 0))
        out = np.empty((max(nt, 1), 3))
        self._chk(self.L.visma_icp_get_color_gradient(self._h, _p(out, _dp), nt))
        return out[:nt].copy()

    def reduce_colored(self, lambda_geometric=0.968):
        """The colored statistics of the last nn_pass -> (stats, ColoredInfo)."""
        st = np.empty(NSTATS); info = CColoredInfo()
        self._chk(self.L.visma_icp_reduce_colored(self._h, float(lambda_geometric), _p(st, _dp), C.byref(info)))
        return st, ColoredInfo(info)

    def run_colored(self, init=None, max_dist=0.05, lambda_geometric=0.968, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        """Colored ICP: a photometric row next to the point-to-plane row of every pair; needs target normals and both
        clouds' colours.  -> Result with .colored (ColoredInfo)."""
        init = _f64(np.eye(4) if init is None else init, (16,))
        out = CResult(); info = CColoredInfo()
        self._chk(self.L.visma_icp_run_colored(self._h, _p(init, _dp), float(max_dist), float(lambda_geometric), int(max_iter),
                                               float(rel_fitness), float(rel_rmse), C.byref(out), C.byref(info)))
        r = Result(out)
        r.colored = ColoredInfo(info)
        return r

    def information_matrix(self, T=None, max_dist=0.05):
        """The information matrix of the edge T between the context's clouds (Choi et al. 2015): sum G^T G over the pairs
        of a pass at T inside max_dist, G = [-hat(q) | I], q the target point -> (6 x 6, K).  Without the identity
        terms of Open3D 0.3.0: [5, 5] == K."""
        T = _f64(np.eye(4) if T is None else T, (16,))
        out = np.empty(36); k = C.c_int64(0)
        self._chk(self.L.visma_icp_information_matrix(self._h, _p(T, _dp), float(max_dist), _p(out, _dp), C.byref(k)))
        return out.reshape(6, 6), k.value

    def reduce_information(self):
        """The information matrix over the pairs of the last nn_pass -> 6 x 6."""
        out = np.empty(36)
        self._chk(self.L.visma_icp_reduce_information(self._h, _p(out, _dp)))
        return out.reshape(6, 6)

    def information_matrices(self, problems):
        """Every edge of a pose graph in one call.  problems: (src, tgt, T, radius) tuples; tuples that pass the same
        target array share its upload -> (n x 6 x 6, K per edge).  Each matrix is bit-equal to set_clouds_f64 +
        information_matrix for that edge."""
        n = len(problems)
        arr = (CProblem * max(n, 1))(); keep = {}

        def once(a):                                     # one C array per Python array: the library groups by pointer
            if id(a) not in keep:
                keep[id(a)] = (a, _f64(a, (-1, 3)))
            return keep[id(a)][1]
        for i, (src, tgt, init, r) in enumerate(problems):
            s = once(src); t = once(tgt)
            arr[i].src_xyz = _p(s, _dp); arr[i].ns = len(s)
            arr[i].tgt_xyz = _p(t, _dp); arr[i].nt = len(t)
            arr[i].init = (C.c_double * 16)(*_f64(np.eye(4) if init is None else init, (16,)))
            arr[i].max_dist = float(r)
        out = np.zeros((max(n, 1), 36)); k = np.zeros(max(n, 1), np.int64)
        self._chk(self.L.visma_icp_information_matrices(self._h, arr, n, _p(out, _dp), _p(k, C.POINTER(C.c_int64))))
        cs, ct = C.c_int64(0), C.c_int64(0)              # the clouds of the last edge the library handled
        self._chk(self.L.visma_icp_get_cloud_sizes(self._h, C.byref(cs), C.byref(ct)))
        self.ns, self.nt = int(cs.value), int(ct.value)
        return out[:n].reshape(n, 6, 6), k[:n]

    # ---- RGB-D odometry (visma_icp.h) ----
    def _odometry_frames(self, src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init):
        frames = (src_gray, src_depth, tgt_gray, tgt_depth)
        if any(isinstance(a, Image) for a in frames):        # resident Images: the *_images entry points
            if not all(isinstance(a, Image) for a in frames):
                raise ValueError("four Images, or four arrays")
            w, h = frames[0].info()[:2]
            k = _f64(intrinsic, (4,)); init = _f64(np.eye(4) if init is None else init, (16,))
            return None, (h, w), k, init, [self._h] + [a._i for a in frames] + [_p(k, _dp), _p(init, _dp)]
        imgs = [np.ascontiguousarray(a, dtype=np.float32) for a in (src_gray, src_depth, tgt_gray, tgt_depth)]
        if imgs[0].ndim != 2 or any(a.shape != imgs[0].shape for a in imgs):
            raise ValueError("four h x w images of one size")
        h, w = imgs[0].shape
        k = _f64(intrinsic, (4,)); init = _f64(np.eye(4) if init is None else init, (16,))
        return imgs, (h, w), k, init, [self._h, w, h] + [_p(a, _fp) for a in imgs] + [_p(k, _dp), _p(init, _dp)]

    def rgbd_odometry(self, src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init=None, method=ODOMETRY_HYBRID, option=None):
        """Open3D's ComputeRGBDOdometry between two frames (h x w fp32 gray and depth in metres; intrinsic [fx, fy, cx, cy])
        -> OdometryResult; unpacks as (success, T, information).  Without success: T = I, information = 0, no exception."""
        option = odometry_option() if option is None else option
        keep, shape, k, init, args = self._odometry_frames(src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init)
        call = self.L.visma_icp_rgbd_odometry if keep is not None else self.L.visma_icp_rgbd_odometry_images
        T = np.empty(16); info = np.empty(36)
        cap = max(1, sum(max(0, option.iterations[i]) for i in range(max(0, min(option.n_levels, 8)))))
        pairs = np.zeros(cap, np.int64)
        res = COdometryResult(); res.pairs = _p(pairs, C.POINTER(C.c_int64)); res.pairs_capacity = cap
        self._chk(call(*args, int(method), C.byref(option), _p(T, _dp), _p(info, _dp), C.byref(res)))
        self._odo_shape = (shape, option.n_levels)   # (the call prepared: its pyramids are the resident ones)
        return OdometryResult(res.success, T.reshape(4, 4), info.reshape(6, 6), res.information_pairs, pairs[:res.iterations].copy())

    def odometry_prepare(self, src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init=None, option=None):
        """Both processed pyramids of a frame pair, resident until the next prepare (what the calls below read)."""
        option = odometry_option() if option is None else option
        keep, shape, k, init, args = self._odometry_frames(src_gray, src_depth, tgt_gray, tgt_depth, intrinsic, init)
        call = self.L.visma_icp_odometry_prepare if keep is not None else self.L.visma_icp_odometry_prepare_images
        self._chk(call(*args, C.byref(option)))
        self._odo_shape = (shape, option.n_levels)

    def image_from_odometry(self, which, level=0):
        """A level of a resident pyramid as an Image, copied device to device (not src_xyz)."""
        which = ODOMETRY_IMAGES.index(which) if isinstance(which, str) else int(which)
        i = C.c_void_p()
        self._chk(self.L.visma_icp_image_from_odometry(self._h, which, int(level), C.byref(i)))
        return Image(self, i)

    def _odometry_level_shape(self, level):
        (h, w), n = getattr(self, "_odo_shape", ((0, 0), 0))
        for _ in range(max(0, min(int(level), 8))):
            h, w = h // 2, w // 2
        return h, w

    def odometry_image(self, which, level=0):
        """A level of a resident pyramid: `which` is an index or a name of ODOMETRY_IMAGES -> h_l x w_l fp32 (src_xyz: x 3)."""
        which = ODOMETRY_IMAGES.index(which) if isinstance(which, str) else int(which)
        h, w = self._odometry_level_shape(level)
        out = np.empty((max(h, 1), max(w, 1), 3) if which == 8 else (max(h, 1), max(w, 1)), np.float32)
        self._chk(self.L.visma_icp_odometry_get_image(self._h, which, int(level), _p(out, _fp)))
        return out

    def odometry_correspondences(self, level=0, T=None):
        """The pairs of a level at T -> (idx, K): idx[v_s * w + u_s] = v_t * w + u_t or -1; np.flatnonzero(idx >= 0) and
        idx[idx >= 0] are the reference's correspondence list."""
        T = _f64(np.eye(4) if T is None else T, (16,))
        h, w = self._odometry_level_shape(level)
        idx = np.empty(max(h * w, 1), np.int32); k = C.c_int64(0)
        self._chk(self.L.visma_icp_odometry_correspondences(self._h, int(level), _p(T, _dp), _p(idx, _ip), C.byref(k)))
        return idx[:h * w], k.value

    def odometry_step(self, level=0, T=None, method=ODOMETRY_HYBRID):
        """One iteration's sums at T -> (stats[38], K, sum r^2); solve_from_stats(stats, SOLVER_GN_EULER) is the update."""
        T = _f64(np.eye(4) if T is None else T, (16,))
        stats = np.empty(38); k = C.c_int64(0); r2 = C.c_double(0)
        self._chk(self.L.visma_icp_odometry_step(self._h, int(level), _p(T, _dp), int(method), _p(stats, _dp), C.byref(k), C.byref(r2)))
        return stats, k.value, r2.value

    def odometry_information(self, T=None):
        """The information matrix of the resident frames at T -> (6 x 6, K)."""
        T = _f64(np.eye(4) if T is None else T, (16,))
        out = np.empty(36); k = C.c_int64(0)
        self._chk(self.L.visma_icp_odometry_information(self._h, _p(T, _dp), _p(out, _dp), C.byref(k)))
        return out.reshape(6, 6), k.value

    # ---- KDTreeFlann (visma_icp.h) ----
    def kdtree(self, xyz):
        """Open3D's KDTreeFlann over xyz (n x 3 f64, n >= 1), resident on the device -> KDTree."""
        p = _f64(xyz, (-1, 3))
        t = C.c_void_p()
        self._chk(self.L.visma_icp_kdtree_create(self._h, _p(p, _dp), len(p), C.byref(t)))
        return KDTree(self, t, len(p))

    # ---- TriangleMesh (visma_icp.h) ----
    def trimesh(self, vertices, triangles, vertex_normals=None, vertex_colors=None, triangle_normals=None):
        """Open3D's TriangleMesh on the device -> TriMesh.  vertices nv x 3 f64, triangles nt x 3 int32 (an index outside
        [0, nv): IcpError), the optional attributes nv x 3 / nt x 3 f64."""
        v = _f64(vertices, (-1, 3))
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        opt = lambda a, n: None if a is None else _f64(a, (n, 3))
        vn, vc, tn = opt(vertex_normals, len(v)), opt(vertex_colors, len(v)), opt(triangle_normals, len(t))
        dp = lambda a: None if a is None else _p(a, _dp)
        m = C.c_void_p()
        self._chk(self.L.visma_icp_trimesh_create(self._h, _p(v, _dp), len(v), dp(vn), dp(vc), _p(t, _ip), len(t), dp(tn), C.byref(m)))
        return TriMesh(self, m)

    # ---- PointCloud (visma_icp.h) ----
    def cloud(self, points, normals=None, colors=None):
        """Open3D's PointCloud on the device -> Cloud.  points n x 3 f64 (n = 0 is a cloud), normals and colors n x 3 f64 or
        None."""
        p = _f64(points, (-1, 3))
        opt = lambda a: None if a is None else _f64(a, (len(p), 3))
        nrm, col = opt(normals), opt(colors)
        dp = lambda a: None if a is None else _p(a, _dp)
        c = C.c_void_p()
        self._chk(self.L.visma_icp_cloud_create(self._h, _p(p, _dp), len(p), dp(nrm), dp(col), C.byref(c)))
        return Cloud(self, c)

    # ---- Image (visma_icp.h) ----
    def image(self, array):
        """Open3D's Image on the device -> Image.  array h x w or h x w x channels of uint8, uint16 or float32."""
        a = np.ascontiguousarray(array)
        if a.dtype not in (np.uint8, np.uint16, np.float32) or a.ndim not in (2, 3):
            raise ValueError("an h x w (x channels) array of uint8, uint16 or float32")
        h, w = a.shape[:2]
        i = C.c_void_p()
        self._chk(self.L.visma_icp_image_create(self._h, w, h, 1 if a.ndim == 2 else a.shape[2], a.dtype.itemsize,
                                                a.ctypes.data_as(C.c_void_p) if a.size else None, C.byref(i)))
        return Image(self, i)

    def render_edges(self, image):
        """The depth-edge image (edge_detection.frag's rule on the metric depth; visma_icp_render has it) of a 1 x float32
        depth Image -> a 1 x uint8 Image"""
        i = C.c_void_p()
        self._chk(self.L.visma_icp_render_edges(self._h, image._i, C.byref(i)))
        return Image(self, i)

    def distance_multiplier(self, intrinsic, w, h):
        """CreateDepthToCameraDistanceMultiplierFloatImage for [fx, fy, cx, cy] and w x h -> Image"""
        k = _f64(intrinsic, (4,))
        i = C.c_void_p()
        self._chk(self.L.visma_icp_image_distance_multiplier(self._h, _p(k, _dp), int(w), int(h), C.byref(i)))
        return Image(self, i)

    def filter_pyramid(self, pyramid, type):
        """FilterImagePyramid -> a list of Images"""
        n = len(pyramid)
        src = (C.c_void_p * max(n, 1))(*[p._i.value for p in pyramid])
        out = (C.c_void_p * max(n, 1))()
        self._chk(self.L.visma_icp_image_filter_pyramid(self._h, src, n, _image_enum(type, IMAGE_FILTERS), out))
        return [Image(self, C.c_void_p(out[l])) for l in range(n)]

    def rgbd(self, color, depth, format="color_and_depth", depth_scale=1000.0, depth_trunc=3.0, convert_rgb_to_intensity=True):
        """CreateRGBDImageFromColorAndDepth / Redwood / TUM / SUN / NYU format (an index or a name of RGBD_FORMATS) of two
        Images -> (color, depth) Images, or (None, None) for images of different sizes (the reference's empty RGBDImage)."""
        c, d = C.c_void_p(), C.c_void_p()
        self._chk(self.L.visma_icp_image_rgbd(self._h, color._i, depth._i, _image_enum(format, RGBD_FORMATS), float(depth_scale),
                                              float(depth_trunc), int(bool(convert_rgb_to_intensity)), C.byref(c), C.byref(d)))
        return (Image(self, c), Image(self, d)) if c.value and d.value else (None, None)

    def cloud_from_depth_image(self, depth, intrinsic, extrinsic=None, depth_scale=1000.0, depth_trunc=1000.0, stride=1):
        """CreatePointCloudFromDepthImage of a resident Image (1 x float32, or 1 x uint16 through depth_scale / depth_trunc) ->
        a resident Cloud: the rows of point_cloud_from_depth.  Any other format: an empty Cloud."""
        k = _f64(intrinsic, (4,)); E = _f64(np.eye(4) if extrinsic is None else extrinsic, (16,))
        c = C.c_void_p()
        self._chk(self.L.visma_icp_cloud_from_depth_image(self._h, depth._i, _p(k, _dp), _p(E, _dp), float(depth_scale), float(depth_trunc),
                                                          int(stride), C.byref(c)))
        return Cloud(self, c)

    def cloud_from_rgbd_images(self, depth, color, intrinsic, extrinsic=None):
        """CreatePointCloudFromRGBDImage of resident Images (depth 1 x float32; color 3 x uint8 or 1 x float32) -> a resident
        Cloud with colours: the rows of point_cloud_from_rgbd.  Any other format: an empty Cloud."""
        k = _f64(intrinsic, (4,)); E = _f64(np.eye(4) if extrinsic is None else extrinsic, (16,))
        c = C.c_void_p()
        self._chk(self.L.visma_icp_cloud_from_rgbd_images(self._h, depth._i, color._i, _p(k, _dp), _p(E, _dp), C.byref(c)))
        return Cloud(self, c)

    # ---- TSDF integration (visma_icp.h) ----
    def tsdf_uniform(self, length, resolution, sdf_trunc, color_type=TSDF_COLOR_NONE, origin=(0.0, 0.0, 0.0)):
        """Open3D's UniformTSDFVolume(length, resolution, sdf_trunc, color_type, origin) on the device -> TsdfVolume.
        color_type: TSDF_COLOR_NONE | TSDF_COLOR_RGB8 | TSDF_COLOR_GRAY32 or "none" | "rgb8" | "gray32"."""
        color_type = _tsdf_color_type(color_type)
        origin = _f64(origin, (3,))
        v = C.c_void_p()
        self._chk(self.L.visma_icp_tsdf_create_uniform(self._h, float(length), int(resolution), float(sdf_trunc), color_type,
                                                       _p(origin, _dp), C.byref(v)))
        return TsdfVolume(self, v, length, resolution, sdf_trunc, color_type, origin)

    def tsdf_scalable(self, voxel_length, sdf_trunc, color_type=TSDF_COLOR_NONE, volume_unit_resolution=16, depth_sampling_stride=4,
                      initial_units=0):
        """Open3D's ScalableTSDFVolume(voxel_length, sdf_trunc, color_type, volume_unit_resolution, depth_sampling_stride) on
        the device -> TsdfVolume; initial_units: the first capacity of its unit pool (0: 256; it doubles when full)."""
        color_type = _tsdf_color_type(color_type)
        v = C.c_void_p()
        self._chk(self.L.visma_icp_tsdf_create_scalable(self._h, float(voxel_length), float(sdf_trunc), color_type,
                                                        int(volume_unit_resolution), int(depth_sampling_stride), int(initial_units), C.byref(v)))
        return TsdfVolume(self, v, float(voxel_length) * int(volume_unit_resolution), volume_unit_resolution, sdf_trunc, color_type, None,
                          scalable=True, voxel_length=voxel_length)

    def _point_cloud_capacity(self, depth, stride):
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if depth.ndim != 2:
            raise ValueError("an h x w depth image")
        h, w = depth.shape
        s = max(int(stride), 1)
        return depth, h, w, max(1, -(-w // s) * -(-h // s))

    def point_cloud_from_depth(self, depth, intrinsic, extrinsic=None, stride=1):
        """Open3D's CreatePointCloudFromDepthImage of a float depth image (metres) -> points (n x 3 f64), row-major pixel
        order; extrinsic: world -> camera (default: the identity)."""
        depth, h, w, cap = self._point_cloud_capacity(depth, stride)
        k = _f64(intrinsic, (4,)); E = _f64(np.eye(4) if extrinsic is None else extrinsic, (16,))
        pts = np.empty((cap, 3)); n = C.c_int64(0)
        self._chk(self.L.visma_icp_point_cloud_from_depth(self._h, w, h, _p(depth, _fp), _p(k, _dp), _p(E, _dp), int(stride),
                                                          _p(pts, _dp), cap, C.byref(n)))
        return pts[:n.value].copy()

    def point_cloud_from_rgbd(self, depth, color, intrinsic, extrinsic=None):
        """Open3D's CreatePointCloudFromRGBDImage: color h x w x 3 uint8 or h x w fp32 -> points, colors (n x 3 f64)."""
        depth, h, w, cap = self._point_cloud_capacity(depth, 1)
        color = np.asarray(color)
        color_type = TSDF_COLOR_RGB8 if color.dtype == np.uint8 else TSDF_COLOR_GRAY32
        color = _tsdf_color_image(color, color_type, (h, w))
        k = _f64(intrinsic, (4,)); E = _f64(np.eye(4) if extrinsic is None else extrinsic, (16,))
        pts, col = np.empty((cap, 3)), np.empty((cap, 3)); n = C.c_int64(0)
        self._chk(self.L.visma_icp_point_cloud_from_rgbd(self._h, w, h, _p(depth, _fp), color.ctypes.data_as(C.c_void_p), color_type,
                                                         _p(k, _dp), _p(E, _dp), _p(pts, _dp), _p(col, _dp), cap, C.byref(n)))
        return pts[:n.value].copy(), col[:n.value].copy()

    # ---- color map optimization (visma_icp.h) ----
    def color_map(self, w, h, n_images, intrinsic, option=None):
        """Open3D's ColorMapOptimization (rigid) as staged calls -> ColorMap.  intrinsic [fx, fy, cx, cy]; option:
        color_map_option(...) (default: Open3D's)."""
        k = _f64(intrinsic, (4,))
        m = C.c_void_p()
        self._chk(self.L.visma_icp_color_map_create(self._h, int(w), int(h), int(n_images), _p(k, _dp),
                                                    None if option is None else C.byref(option), C.byref(m)))
        return ColorMap(self, m, w, h, n_images)

    def color_map_non_rigid(self, w, h, n_images, intrinsic, option=None):
        """The NON-RIGID ColorMapOptimization as staged calls -> ColorMap with a warping field per image (anchor_shape, flow,
        set_flow, cell_sums, step_non_rigid).  The anchors and the weight come from `option`, whatever its flag says."""
        k = _f64(intrinsic, (4,))
        m = C.c_void_p()
        self._chk(self.L.visma_icp_color_map_create_non_rigid(self._h, int(w), int(h), int(n_images), _p(k, _dp),
                                                              None if option is None else C.byref(option), C.byref(m)))
        return ColorMap(self, m, w, h, n_images)

    def color_map_optimization_non_rigid(self, vertices, depths, colors, intrinsic, extrinsics, option=None):
        """The non-rigid ColorMapOptimization in one call (arguments as color_map_optimization)
        -> (refined extrinsics n x 4 x 4, vertex colours m x 3, flows n x (anchor_w anchor_h 2))."""
        depths = np.ascontiguousarray(depths, dtype=np.float32)
        colors = np.ascontiguousarray(colors, dtype=np.uint8)
        if depths.ndim != 3 or colors.shape != depths.shape + (3,):
            raise ValueError("depths n x h x w and colors n x h x w x 3")
        n, h, w = depths.shape
        anchors = 16 if option is None else int(option.number_of_vertical_anchors)
        if anchors < 2 or anchors > 64:
            raise IcpError(1, "number_of_vertical_anchors outside 2 .. 64")
        aw = int(np.ceil(float(w) / (float(h) / (anchors - 1))) + 1)
        v = _f64(vertices, (-1, 3)); k = _f64(intrinsic, (4,))
        E = _f64(extrinsics, (n * 16,)).copy()
        out, flow = np.empty((len(v), 3)), np.empty((n, aw * anchors * 2))
        self._chk(self.L.visma_icp_color_map_optimization_non_rigid(self._h, w, h, n, _p(k, _dp), _p(depths, _fp),
                                                                    colors.ctypes.data_as(C.POINTER(C.c_uint8)), _p(E, _dp), _p(v, _dp),
                                                                    len(v), None if option is None else C.byref(option), _p(out, _dp),
                                                                    _p(flow, _dp)))
        return E.reshape(n, 4, 4), out, flow

    def color_map_optimization(self, vertices, depths, colors, intrinsic, extrinsics, option=None):
        """ColorMapOptimization in one call: depths n x h x w fp32, colors n x h x w x 3 uint8, extrinsics n x 4 x 4
        -> (refined extrinsics n x 4 x 4, vertex colours m x 3)."""
        depths = np.ascontiguousarray(depths, dtype=np.float32)
        colors = np.ascontiguousarray(colors, dtype=np.uint8)
        if depths.ndim != 3 or colors.shape != depths.shape + (3,):
            raise ValueError("depths n x h x w and colors n x h x w x 3")
        n, h, w = depths.shape
        v = _f64(vertices, (-1, 3)); k = _f64(intrinsic, (4,))
        E = _f64(extrinsics, (n * 16,)).copy()
        out = np.empty((len(v), 3))
        self._chk(self.L.visma_icp_color_map_optimization(self._h, w, h, n, _p(k, _dp), _p(depths, _fp),
                                                          colors.ctypes.data_as(C.POINTER(C.c_uint8)), _p(E, _dp), _p(v, _dp), len(v),
                                                          None if option is None else C.byref(option), _p(out, _dp)))
        return E.reshape(n, 4, 4), out

    def iterate(self, T, max_dist, steps, solver=SOLVER_KABSCH, with_scaling=False):
        """Exactly `steps` fixed iterations from T; returns (T_new, Result of last pass)."""
        T = _f64(np.eye(4) if T is None else T, (16,)).copy()
        out = CResult()
        self._chk(self.L.visma_icp_iterate(self._h, _p(T, _dp), float(max_dist), int(steps),
                                           int(solver), int(bool(with_scaling)), C.byref(out)))
        return T.reshape(4, 4), Result(out)

    def run_point_to_plane(self, init=None, max_dist=0.05, max_iter=30, rel_fitness=1e-6,
                           rel_rmse=1e-6):
        init = _f64(np.eye(4) if init is None else init, (16,))
        out = CResult()
        self._chk(self.L.visma_icp_run_point_to_plane(self._h, _p(init, _dp), float(max_dist),
                                                      int(max_iter), float(rel_fitness),
                                                      float(rel_rmse), C.byref(out)))
        return Result(out)

    def run_yaw_sweep(self, level, max_dist, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                      solver=SOLVER_KABSCH):
        best = CResult(); bl = C.c_int(-1); per = (CResult * level)()
        self._chk(self.L.visma_icp_run_yaw_sweep(self._h, int(level), float(max_dist),
                                                 int(max_iter), float(rel_fitness),
                                                 float(rel_rmse), int(solver), C.byref(best),
                                                 C.byref(bl), per))
        return Result(best), bl.value, [Result(p) for p in per]

    def run_yaw_sweep_point_to_plane(self, level, max_dist, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        best = CResult(); bl = C.c_int(-1); per = (CResult * level)()
        self._chk(self.L.visma_icp_run_yaw_sweep_point_to_plane(self._h, int(level), float(max_dist), int(max_iter),
                                                                float(rel_fitness), float(rel_rmse), C.byref(best),
                                                                C.byref(bl), per))
        return Result(best), bl.value, [Result(p) for p in per]

    @staticmethod
    def make_batch(problems):
        """The visma_icp_problem array of (src, tgt, init, radius) tuples, built once: a caller that runs the
        same batch again (bench.py) does not pay the ctypes marshalling inside its timed region."""
        n = len(problems)
        arr = (CProblem * max(n, 1))(); keep = []
        for i, (src, tgt, init, r) in enumerate(problems):
            s = _f64(src, (-1, 3)); t = _f64(tgt, (-1, 3)); keep += [s, t]
            arr[i].src_xyz = _p(s, _dp); arr[i].ns = len(s)
            arr[i].tgt_xyz = _p(t, _dp); arr[i].nt = len(t)
            arr[i].init = (C.c_double * 16)(*_f64(np.eye(4) if init is None else init, (16,)))
            arr[i].max_dist = float(r)
        return (arr, n, keep, (CResult * max(n, 1))())

    def run_batch(self, problems, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                  solver=SOLVER_KABSCH):
        """problems: (src, tgt, init, radius) tuples, or the value of make_batch()."""
        arr, n, _keep, out = problems if (isinstance(problems, tuple) and len(problems) == 4 and
                                          isinstance(problems[1], int)) else self.make_batch(problems)
        self._chk(self.L.visma_icp_run_batch(self._h, arr, n, int(max_iter), float(rel_fitness),
                                             float(rel_rmse), int(solver), out))
        return [Result(out[i]) for i in range(n)]

    def run_batch_point_to_plane(self, problems, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        """problems: (src, tgt, tgt_normals or None, init, radius) -- the point-to-plane estimator, all in flight."""
        n = len(problems)
        arr = (CProblem * max(n, 1))(); nrm = (_dp * max(n, 1))(); keep = []
        for i, (src, tgt, normals, init, r) in enumerate(problems):
            s = _f64(src, (-1, 3)); t = _f64(tgt, (-1, 3)); keep += [s, t]
            arr[i].src_xyz = _p(s, _dp); arr[i].ns = len(s)
            arr[i].tgt_xyz = _p(t, _dp); arr[i].nt = len(t)
            arr[i].init = (C.c_double * 16)(*_f64(np.eye(4) if init is None else init, (16,)))
            arr[i].max_dist = float(r)
            if normals is not None:
                q = _f64(normals, (-1, 3)); keep.append(q)
                assert len(q) == len(t)
                nrm[i] = _p(q, _dp)
        out = (CResult * max(n, 1))()
        self._chk(self.L.visma_icp_run_batch_point_to_plane(self._h, arr, nrm, n, int(max_iter), float(rel_fitness),
                                                            float(rel_rmse), out))
        return [Result(out[i]) for i in range(n)]

    def estimate_normals(self, xyz, knn=30, radius=None, normals=None):
        """open3d::EstimateNormals on the GPU.  radius None: KNN(knn); knn None: Radius(radius); both: Hybrid."""
        p = _f64(xyz, (-1, 3)); n = len(p)
        nin = None if normals is None else _f64(normals, (-1, 3))
        kind = 0 if radius is None else (1 if knn is None else 2)
        out = np.empty((max(n, 1), 3))
        self._chk(self.L.visma_icp_estimate_normals(self._h, _p(p, _dp), n, None if nin is None else _p(nin, _dp),
                                                    kind, int(knn or 0), float(radius or 0.0), _p(out, _dp)))
        return out[:n].copy()

    def color_gradient(self, xyz, normals, colors, radius, max_nn=30):
        """The colour gradient per point of colored ICP (ColoredICP.cpp:74-137) for any cloud -> (n, 3)."""
        p = _f64(xyz, (-1, 3)); n = len(p)
        nn = _f64(normals, (-1, 3)); cc = _f64(colors, (-1, 3))
        if len(nn) != n or len(cc) != n:
            raise ValueError("color_gradient: one normal and one colour per point")
        out = np.empty((max(n, 1), 3))
        self._chk(self.L.visma_icp_color_gradient(self._h, _p(p, _dp), n, _p(nn, _dp), _p(cc, _dp), float(radius), int(max_nn),
                                                  _p(out, _dp)))
        return out[:n].copy()

    def compute_fpfh(self, xyz, normals, knn=100, radius=None, second_pass=None, timing=None):
        """open3d::ComputeFPFHFeature on the GPU -> (n, 33), row i the reference's column i.  radius None: KNN(knn); else
        Hybrid(radius, knn).  second_pass (measurement): 1 keeps the lists of the first pass, 2 rebuilds them; timing: a
        list that receives [grid ms, SPFH ms, FPFH ms]."""
        p = _f64(xyz, (-1, 3)); n = len(p)
        nn = _f64(normals, (-1, 3))
        if len(nn) != n:
            raise ValueError("compute_fpfh: one normal per point")
        out = np.empty((max(n, 1), FPFH_DIM))
        kind, r = (0, 0.0) if radius is None else (2, float(radius))
        if second_pass is None and timing is None:
            self._chk(self.L.visma_icp_compute_fpfh(self._h, _p(p, _dp), n, _p(nn, _dp), kind, int(knn), r, _p(out, _dp)))
        else:
            ms = np.zeros(3)
            self._chk(self.L.visma_icp_compute_fpfh_probe(self._h, _p(p, _dp), n, _p(nn, _dp), kind, int(knn), r, _p(out, _dp),
                                                          int(second_pass or 0), _p(ms, _dp)))
            if timing is not None:
                timing[:] = list(ms)
        return out[:n].copy()

    def match_features(self, fa, fb, timing=None):
        """For every row of fb the row of fa at the smallest squared distance (flann's L2, lowest index on ties)
        -> (indices (nb,) int32, -1 where none; d2 (nb,))."""
        b = _f64(fb); b = b.reshape(len(b), -1) if b.ndim != 2 else b
        a = _f64(fa); a = a.reshape(len(a), -1) if a.ndim != 2 else a
        dim = b.shape[1] if len(b) else a.shape[1]
        if len(a) and len(b) and a.shape[1] != b.shape[1]:
            raise ValueError("match_features: both sets need the same dimension")
        nn = np.empty(max(len(b), 1), np.int32); d2 = np.empty(max(len(b), 1))
        ms = C.c_double(0.0)
        self._chk(self.L.visma_icp_match_features_probe(self._h, _p(a, _dp), len(a), _p(b, _dp), len(b), int(dim), _p(nn, _ip),
                                                        _p(d2, _dp), C.byref(ms)))
        if timing is not None:
            timing[:] = [ms.value]
        return nn[:len(b)].copy(), d2[:len(b)].copy()

    def fgr_correspondences(self, src, src_fpfh, tgt, tgt_fpfh, option=None, seed=0, triples=None):
        """Fast global registration up to its tuple test -> ((k, 2) int32 pairs (source, target), FgrInfo)."""
        s = _f64(src, (-1, 3)); t = _f64(tgt, (-1, 3))
        fs = _f64(src_fpfh, (-1, FPFH_DIM)); ft = _f64(tgt_fpfh, (-1, FPFH_DIM))
        if len(fs) != len(s) or len(ft) != len(t):
            raise ValueError("fgr_correspondences: one feature row per point")
        o = option if option is not None else fgr_option()
        tr, ntr, trp = _fgr_triples(triples)
        cap = 3 * max(1, min(int(o.maximum_tuple_count), 100 * min(len(s), len(t))))
        si = np.empty(cap, np.int32); ti = np.empty(cap, np.int32)
        k = C.c_int64(0); info = CFgrInfo()
        self._chk(self.L.visma_icp_fgr_correspondences(self._h, _p(s, _dp), len(s), _p(fs, _dp), _p(t, _dp), len(t), _p(ft, _dp),
                                                       C.byref(o), int(seed), trp, ntr, _p(si, _ip), _p(ti, _ip), cap,
                                                       C.byref(k), C.byref(info)))
        return np.stack([si[:k.value], ti[:k.value]], 1), FgrInfo(info)

    def fgr_optimize(self, src, tgt, src_idx, tgt_idx, option=None):
        """The module's fgr_optimize (host only; here for symmetry with the C++ names)."""
        return fgr_optimize(src, tgt, src_idx, tgt_idx, option)

    def fast_global_registration(self, src, src_fpfh, tgt, tgt_fpfh, option=None, seed=0, triples=None):
        """open3d::FastGlobalRegistration -> (T source-to-target (4, 4), FgrInfo)."""
        s = _f64(src, (-1, 3)); t = _f64(tgt, (-1, 3))
        fs = _f64(src_fpfh, (-1, FPFH_DIM)); ft = _f64(tgt_fpfh, (-1, FPFH_DIM))
        if len(fs) != len(s) or len(ft) != len(t):
            raise ValueError("fast_global_registration: one feature row per point")
        o = option if option is not None else fgr_option()
        tr, ntr, trp = _fgr_triples(triples)
        T = np.empty(16); info = CFgrInfo()
        self._chk(self.L.visma_icp_fast_global_registration(self._h, _p(s, _dp), len(s), _p(fs, _dp), _p(t, _dp), len(t),
                                                            _p(ft, _dp), C.byref(o), int(seed), trp, ntr, _p(T, _dp),
                                                            C.byref(info)))
        return T.reshape(4, 4), FgrInfo(info)

    def ransac_hypotheses(self, src, tgt, pair_tgt, option=None, seed=0, draws=None, first_trial=0, n_trials=0, src_normals=None,
                          tgt_normals=None, pair_src=None):
        """The hypothesis stage of RANSAC on the GPU, trials [first_trial, first_trial + n_trials): pair k is
        (pair_src[k], pair_tgt[k]) or, without pair_src, (k, pair_tgt[k]) -> (verdict (n,) int8, T (n, 4, 4))."""
        keep, o, verdict, T, args = _ransac_hyp_args(src, tgt, src_normals, tgt_normals, pair_src, pair_tgt, option, draws,
                                                     first_trial, n_trials)
        self._chk(self.L.visma_icp_ransac_hypotheses(self._h, *args, int(seed), None if keep[6] is None else _p(keep[6], _ip),
                                                     int(first_trial), int(n_trials), _p(verdict, C.POINTER(C.c_int8)), _p(T, _dp)))
        return verdict[:int(n_trials)].copy(), T[:int(n_trials)].reshape(-1, 4, 4).copy()

    def ransac_hypotheses_probe(self, src, tgt, pair_tgt, option=None, seed=0, n_trials=0, src_normals=None, tgt_normals=None,
                                pair_src=None):
        """Measurement: the hypothesis stage over trials [0, n_trials) without its rows
        -> ([passed, rejected before, rejected after], device ms)."""
        keep, o, _, _, args = _ransac_hyp_args(src, tgt, src_normals, tgt_normals, pair_src, pair_tgt, option, None, 0, 0)
        counts = np.zeros(3, np.int64); ms = C.c_double(0.0)
        self._chk(self.L.visma_icp_ransac_hypotheses_probe(self._h, *args, int(seed), int(n_trials),
                                                           _p(counts, C.POINTER(C.c_int64)), C.byref(ms)))
        return [int(c) for c in counts], ms.value

    def registration_ransac_feature_matching(self, src, src_feat, tgt, tgt_feat, max_dist, option=None, seed=0, draws=None,
                                             src_normals=None, tgt_normals=None):
        """open3d::RegistrationRANSACBasedOnFeatureMatching (point-to-point, the three built-in checkers through `option`)
        -> Result with .ransac (RansacInfo).  The context then holds the pair and the pass at the returned pose."""
        s = _f64(src, (-1, 3)); t = _f64(tgt, (-1, 3))
        fs = _f64(src_feat); ft = _f64(tgt_feat)
        fs = fs.reshape(len(s), -1) if len(s) else fs; ft = ft.reshape(len(t), -1) if len(t) else ft
        if fs.ndim != 2 or ft.ndim != 2 or fs.shape[1] != ft.shape[1]:
            raise ValueError("registration_ransac_feature_matching: one feature row per point, one dimension")
        sn = None if src_normals is None else _f64(src_normals, (-1, 3))
        tn = None if tgt_normals is None else _f64(tgt_normals, (-1, 3))
        o = option if option is not None else ransac_option()
        d, nd, dp_ = _ransac_draws(draws, o.ransac_n)
        out = CResult(); info = CRansacInfo()
        self._chk(self.L.visma_icp_registration_ransac_feature_matching(
            self._h, _p(s, _dp), len(s), _p(fs, _dp), _p(t, _dp), len(t), _p(ft, _dp), int(fs.shape[1]),
            None if sn is None else _p(sn, _dp), None if tn is None else _p(tn, _dp), float(max_dist), C.byref(o), int(seed), dp_, nd,
            C.byref(out), C.byref(info)))
        self.ns, self.nt = len(s), len(t)
        r = Result(out)
        r.ransac = RansacInfo(info)
        return r

    def registration_ransac_correspondence(self, src, tgt, pairs, max_dist, ransac_n=6, max_iteration=1000, max_validation=1000,
                                           seed=0, draws=None):
        """open3d::RegistrationRANSACBasedOnCorrespondence over pairs (K, 2) (source index, target index) -> Result with
        .ransac; fitness and rmse are those of the pair list."""
        s = _f64(src, (-1, 3)); t = _f64(tgt, (-1, 3))
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        si = np.ascontiguousarray(pr[:, 0]); ti = np.ascontiguousarray(pr[:, 1])
        d, nd, dp_ = _ransac_draws(draws, ransac_n)
        out = CResult(); info = CRansacInfo()
        self._chk(self.L.visma_icp_registration_ransac_correspondence(
            self._h, _p(s, _dp), len(s), _p(t, _dp), len(t), _p(si, _ip), _p(ti, _ip), len(si), float(max_dist), int(ransac_n),
            int(max_iteration), int(max_validation), int(seed), dp_, nd, C.byref(out), C.byref(info)))
        r = Result(out)
        r.ransac = RansacInfo(info)
        return r

    def voxel_down_sample(self, xyz, voxel_size, normals=None, colors=None):
        """open3d::VoxelDownSample on the GPU -> (points, normals, colors), voxels in ascending index order."""
        p = _f64(xyz, (-1, 3)); n = len(p)
        nn = None if normals is None else _f64(normals, (-1, 3))
        cc = None if colors is None else _f64(colors, (-1, 3))
        op = np.empty((max(n, 1), 3)); on = np.empty((max(n, 1), 3)); oc = np.empty((max(n, 1), 3))
        m = C.c_int64(0)
        self._chk(self.L.visma_icp_voxel_down_sample(
            self._h, _p(p, _dp), n, None if nn is None else _p(nn, _dp), None if cc is None else _p(cc, _dp),
            float(voxel_size), _p(op, _dp), _p(on, _dp), _p(oc, _dp), C.byref(m)))
        m = m.value
        return op[:m].copy(), (None if nn is None else on[:m].copy()), (None if cc is None else oc[:m].copy())

    def sample_mesh(self, V, F, n, quirks=False, seed=0, uniforms=None):
        """feh::SamplePointCloudFromMesh on the GPU -> (m, 3) points, m <= n."""
        V = _f64(V, (-1, 3)); F = np.ascontiguousarray(F, np.int32).reshape(-1, 3)
        u = None if uniforms is None else _f64(uniforms, (-1, 3))
        if u is not None:
            n = len(u)
        out = np.empty((max(n, 1), 3)); m = C.c_int64(0)
        self._chk(self.L.visma_icp_sample_mesh(self._h, _p(V, _dp), len(V), _p(F, _ip), len(F), int(n),
                                               int(bool(quirks)), int(seed), None if u is None else _p(u, _dp),
                                               _p(out, _dp), C.byref(m)))
        return out[:m.value].copy()

    def point_mesh_distance(self, P, V, F):
        """-> (d2, face, closest) of every query point against the triangle mesh."""
        P = _f64(P, (-1, 3)); V = _f64(V, (-1, 3)); F = np.ascontiguousarray(F, np.int32).reshape(-1, 3)
        d2 = np.empty(max(len(P), 1)); face = np.empty(max(len(P), 1), np.int32); cl = np.empty((max(len(P), 1), 3))
        self._chk(self.L.visma_icp_point_mesh_distance(self._h, _p(P, _dp), len(P), _p(V, _dp), len(V),
                                                       _p(F, _ip), len(F), _p(d2, _dp), _p(face, _ip), _p(cl, _dp)))
        return d2[:len(P)], face[:len(P)], cl[:len(P)]

    def point_cloud_distance(self, src, tgt):
        """open3d::ComputePointCloudToPointCloudDistance on the GPU: the distance of every source point to the nearest
        target point (no radius; 0 for an empty target)."""
        src = _f64(src, (-1, 3)); tgt = _f64(tgt, (-1, 3))
        d = np.empty(max(len(src), 1))
        self._chk(self.L.visma_icp_point_cloud_distance(self._h, _p(src, _dp), len(src), _p(tgt, _dp), len(tgt),
                                                        _p(d, _dp)))
        return d[:len(src)]

    def nearest_neighbor_distance(self, xyz):
        """open3d::ComputePointCloudNearestNeighborDistance on the GPU: the distance of every point to the nearest
        other point of the cloud (0 for a duplicate, [0.0] for one point)."""
        p = _f64(xyz, (-1, 3))
        d = np.empty(max(len(p), 1))
        self._chk(self.L.visma_icp_nearest_neighbor_distance(self._h, _p(p, _dp), len(p), _p(d, _dp)))
        return d[:len(p)]

    def last_mesh_kernel_ms(self):
        """-> (query kernel ms, search-structure build ms) of the last mesh-distance call."""
        ms, bms = C.c_double(0), C.c_double(0)
        self._chk(self.L.visma_icp_last_mesh_kernel_ms(self._h, C.byref(ms), C.byref(bms)))
        return ms.value, bms.value

    def set_search_precision(self, mode):
        """'exact' (default; alias 'auto': fp32 ranking, near-ties re-ranked in f64) | 'f32' | 'f64';
        before set_clouds_f64."""
        self._chk(self.L.visma_icp_set_search_precision(self._h, {"f32": 0, "auto": 1, "exact": 1, "f64": 2}[mode]))

    def search_mode_used(self):
        """'f32' | 'exact' | 'f64': the arithmetic of the last pass."""
        v = C.c_int(0)
        self._chk(self.L.visma_icp_get_search_precision_used(self._h, C.byref(v)))
        return {0: "f32", 1: "exact", 2: "f64"}[v.value]

    def search_is_f64(self):
        """True when the last pass returned the reference's own (f64) correspondences."""
        return self.search_mode_used() != "f32"

    def set_mesh_search(self, method):
        """'auto' | 'brute' | 'bvh'"""
        self._chk(self.L.visma_icp_set_mesh_search(self._h, {"auto": 0, "brute": 1, "bvh": 2}[method]))

    def measure_surface_error(self, Vs, Fs, Vt, Ft, num_samples, quirks=False, seed=0):
        Vs = _f64(Vs, (-1, 3)); Fs = np.ascontiguousarray(Fs, np.int32).reshape(-1, 3)
        Vt = _f64(Vt, (-1, 3)); Ft = np.ascontiguousarray(Ft, np.int32).reshape(-1, 3)
        out = np.empty(5)
        self._chk(self.L.visma_icp_measure_surface_error(self._h, _p(Vs, _dp), len(Vs), _p(Fs, _ip), len(Fs),
                                                         _p(Vt, _dp), len(Vt), _p(Ft, _ip), len(Ft),
                                                         int(num_samples), int(bool(quirks)), int(seed), _p(out, _dp)))
        return dict(zip(("mean", "std", "median", "min", "max"), out))

    # ---- options ----
    def set_nn_mode(self, mode):
        self._chk(self.L.visma_icp_set_nn_mode(self._h, int(mode)))

    def nn_mode_used(self):
        m = C.c_int(0)
        self._chk(self.L.visma_icp_get_nn_mode_used(self._h, C.byref(m)))
        return m.value

    def search_kernel_used(self):
        """'brute' | 'serial' (lane-serial grid search) | 'warm' (warm-started wave-cooperative grid search) | 'ring' (cells
        smaller than the radius, searched in rings: grid_ring.hip)."""
        v = C.c_int(0)
        self._chk(self.L.visma_icp_get_search_kernel_used(self._h, C.byref(v)))
        return {0: "brute", 1: "serial", 2: "warm", 3: "ring"}[v.value]

    def forget_winners(self):
        """The next pass runs like the first of a new registration (no warm start)."""
        self._chk(self.L.visma_icp_forget_winners(self._h))

    def set_persistent(self, on=True, timeout_ms=0.0):
        """the persistent launch of a host loop (default on); timeout_ms > 0: the launch's patience"""
        self._chk(self.L.visma_icp_set_persistent(self._h, int(bool(on)), float(timeout_ms)))

    def persistent_info(self):
        """what the persistent launches of this context's host loops did so far (visma_icp_get_persistent_info)"""
        t = CPersistentInfo()
        t.struct_size = C.sizeof(CPersistentInfo)
        self._chk(self.L.visma_icp_get_persistent_info(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in CPersistentInfo._fields_ if k != "reserved"}

    def sweep_info(self):
        """persistent sweep launches of this context's device-resident loops: started / gave up (visma_icp_get_sweep_info)"""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._chk(self.L.visma_icp_get_sweep_info(self._h, C.byref(a), C.byref(b)))
        return {"launches": a.value, "aborts": b.value}

    def set_ring_search(self, mode=-1):
        """cells smaller than the radius, searched in rings (grid_ring.hip): -1 by occupancy, 0 never, 1 whenever possible"""
        self._chk(self.L.visma_icp_set_ring_search(self._h, int(mode)))

    def ring_search(self):
        """what the current grid is (visma_icp_get_ring_search): rings > 0 = the ring search"""
        r, c, o = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        self._chk(self.L.visma_icp_get_ring_search(self._h, C.byref(r), C.byref(c), C.byref(o)))
        return {"rings": r.value, "cell": c.value, "occupancy": o.value}

    def set_rotation_axis(self, axis=None):
        """every solve of this context rotates about `axis` only (target frame, e.g. (0, 1, 0) for a gravity-aligned scan)
        plus a free translation; None clears it (the default: the unconstrained solves).  visma_icp_set_rotation_axis"""
        if axis is None:
            self._chk(self.L.visma_icp_set_rotation_axis(self._h, None))
        else:
            a = _f64(axis, (3,))
            self._chk(self.L.visma_icp_set_rotation_axis(self._h, _p(a, _dp)))

    def rotation_axis(self):
        """the unit axis in use, or None"""
        a = np.zeros(3)
        e = C.c_int(0)
        self._chk(self.L.visma_icp_get_rotation_axis(self._h, _p(a, _dp), C.byref(e)))
        return a if e.value else None

    def test_stall_command(self, nth, ms):
        self._chk(self.L.visma_icp_test_stall_command(self._h, int(nth), float(ms)))

    def set_device_loop(self, on=True):
        """True: on-device loop, False: host loop, None: automatic (default)."""
        self._chk(self.L.visma_icp_set_device_loop(self._h, -1 if on is None else int(bool(on))))

    def set_profiling(self, on=True):
        """False/0 off, True/1 every launch, n > 1 every n-th ICP pass."""
        self._chk(self.L.visma_icp_set_profiling(self._h, int(on)))

    def get_timing(self, reset=False):
        t = CTiming()
        self._chk(self.L.visma_icp_get_timing(self._h, C.byref(t), int(bool(reset))))
        d = {k: getattr(t, k) for k, _ in CTiming._fields_}
        d["tile_phase_cycles"] = [float(x) for x in d["tile_phase_cycles"]]
        return d

    def launch_config(self):
        a = C.c_int(); b = C.c_int()
        self._chk(self.L.visma_icp_get_launch_config(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- multi-GPU ----
    def comm_ipc_export(self):
        """-> 64-byte handle of this context's all-reduce mailbox (all-gather them, then comm_ipc_init)."""
        buf = C.create_string_buffer(IPC_HANDLE_BYTES)
        self._chk(self.L.visma_icp_comm_ipc_export(self._h, buf))
        return buf.raw

    def comm_ipc_init(self, rank, nranks, handles):
        """handles: the nranks exported handles in rank order (bytes, nranks * 64)."""
        raw = b"".join(bytes(h) for h in handles) if not isinstance(handles, (bytes, bytearray)) else bytes(handles)
        assert len(raw) == nranks * IPC_HANDLE_BYTES
        buf = C.create_string_buffer(raw, len(raw))
        self._chk(self.L.visma_icp_comm_ipc_init(self._h, int(rank), int(nranks), buf))

    def comm_init(self, rank, nranks, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        self._chk(self.L.visma_icp_comm_init(self._h, int(rank), int(nranks), buf))

    def set_allreduce(self, fn, rank, nranks):
        """fn(np.ndarray[38]) must sum in place across ranks (host all-reduce)."""
        def tramp(_user, ptr, n):
            try:
                a = np.ctypeslib.as_array(ptr, shape=(n,))
                fn(a)
                return 0
            except Exception:
                return 1
        cb = ALLREDUCE_FN(tramp)
        self._keep.append(cb)
        self._chk(self.L.visma_icp_set_allreduce(self._h, cb, None, int(rank), int(nranks)))

    def set_target_shard(self, global_offset, global_nt, centre=None):
        """Target-sharded rank: this context holds targets [offset, offset + nt) of `global_nt`.
        Call before set_clouds_f64; `centre` must be the same on every rank."""
        c = None if centre is None else _f64(centre, (3,))
        self._chk(self.L.visma_icp_set_target_shard(self._h, int(global_offset), int(global_nt),
                                                    None if c is None else _p(c, _dp)))

    def set_minreduce(self, fn):
        """fn(np.ndarray[uint64, n]) must take the element-wise minimum across ranks in place."""
        def tramp(_user, ptr, n):
            try:
                fn(np.ctypeslib.as_array(ptr, shape=(n,)))
                return 0
            except Exception:
                return 1
        cb = MINREDUCE_FN(tramp)
        self._keep.append(cb)
        self._chk(self.L.visma_icp_set_minreduce(self._h, cb, None))

    def set_global_source_count(self, n):
        self._chk(self.L.visma_icp_set_global_source_count(self._h, int(n)))


class Corpus:
    """visma_icp_run_corpus: items = [(model_xyz, scene_xyz), ...] (arrays kept alive here), one host thread per
    context pulls chunks from a counter.  `counter_address`: address of an int64 in shared memory when ranks in
    other processes pull from the same queue (else a private counter)."""

    def __init__(self, items, level=24, max_dist=0.05, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                 solver=SOLVER_KABSCH, chunk=8):
        self.L = load()
        self._keep = [(_f64(m, (-1, 3)), _f64(s, (-1, 3))) for m, s in items]
        self.n = len(self._keep)
        self.items = (CCorpusItem * max(self.n, 1))()
        for i, (m, s) in enumerate(self._keep):
            self.items[i] = CCorpusItem(_p(m, _dp), len(m), _p(s, _dp), len(s))
        self.params = CCorpusParams(int(level), float(max_dist), int(max_iter), float(rel_fitness), float(rel_rmse),
                                    int(solver), int(chunk))
        self.results = (CCorpusResult * max(self.n, 1))()

    def run(self, ctxs, counter_address=None):
        """-> list of (Result best, best_level, device, iterations_all_starts) per item (device -1: another process's)."""
        arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
        err = C.create_string_buffer(512)
        cnt = C.cast(C.c_void_p(counter_address), C.POINTER(C.c_int64)) if counter_address else None
        rc = self.L.visma_icp_run_corpus(arr, len(ctxs), self.items, self.n, C.byref(self.params), cnt, self.results, err, 512)
        if rc != 0:
            raise IcpError(rc, err.value.decode(errors="replace"))
        return [(Result(self.results[i].best), int(self.results[i].best_level), int(self.results[i].device),
                 int(self.results[i].iterations_all_starts)) for i in range(self.n)]


def run_batch_multi(ctxs, problems, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, solver=SOLVER_KABSCH):
    """visma_icp_run_batch_multi: one batch over several worker contexts (same GPU or several).  problems: the value
    of Context.make_batch() (or a list of (src, tgt, init, radius) tuples) -> list of Result."""
    L = load()
    arr, n, _keep, out = problems if (isinstance(problems, tuple) and len(problems) == 4 and
                                      isinstance(problems[1], int)) else ctxs[0].make_batch(problems)
    h = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    err = C.create_string_buffer(512)
    rc = L.visma_icp_run_batch_multi(h, len(ctxs), arr, n, int(max_iter), float(rel_fitness), float(rel_rmse), int(solver),
                                     out, err, 512)
    if rc != 0:
        raise IcpError(rc, err.value.decode(errors="replace"))
    return [Result(out[i]) for i in range(n)]


def set_persistent_cu_share(share):
    """per process: the largest part of a device's workgroup slots a persistent launch may hold (0 < share <= 1)"""
    rc = load().visma_icp_set_persistent_cu_share(float(share))
    if rc != 0:
        raise IcpError(rc, "visma_icp_set_persistent_cu_share(%r)" % (share,))


def device_count():
    """HIP devices visible to this process, asked through the library (no torch import: its bundled ROCm
    libraries, RCCL among them, must not be what a later dlopen in this process resolves to)."""
    return int(load().visma_icp_device_count())


def comm_unique_id():
    L = load()
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    rc = L.visma_icp_comm_unique_id(buf)
    if rc != OK:
        msg = L.visma_icp_last_error(None)
        raise IcpError(rc, msg.decode() if msg else "")
    return bytes(buf.raw)


def error_metric(errors):
    L = load()
    e = _f64(errors, (-1,)); out = np.empty(5)
    rc = L.visma_icp_error_metric(_p(e, _dp), len(e), _p(out, _dp))
    if rc != OK:
        raise IcpError(rc, "error_metric")
    return dict(zip(("mean", "std", "median", "min", "max"), out))


def selftest_neighbor_lists(xyz, search_type, cap, radius=0.0, list_kind=0):
    """(tests) visma_icp_selftest_neighbor_lists: the neighbour lists of nn_list.h as the GPU builds them -> idx (n, cap)
    int32 padded with -1, d2 (n, cap) padded with +inf, cnt (n,); search_type 1 (Radius, the counting pass): cnt alone."""
    L = load()
    p = _f64(xyz, (-1, 3)); n = len(p)
    cnt = np.full(n, -7, np.int32)
    if search_type == 1:
        idx = d2 = None
    else:
        idx = np.full((n, max(cap, 0)), -7, np.int32); d2 = np.full((n, max(cap, 0)), np.nan)
    rc = L.visma_icp_selftest_neighbor_lists(_p(p, _dp), n, search_type, cap, radius, list_kind,
                                             None if idx is None else _p(idx, _ip), None if d2 is None else _p(d2, _dp),
                                             _p(cnt, _ip))
    if rc != OK:
        raise IcpError(rc, "selftest_neighbor_lists")
    return cnt if search_type == 1 else (idx, d2, cnt)


class CIoCloud(C.Structure):
    _fields_ = [("n", C.c_int64), ("xyz", _dp), ("n_normals", C.c_int64), ("normals", _dp),
                ("n_colors", C.c_int64), ("colors", _dp), ("n_faces", C.c_int64), ("faces", _ip)]


class IoError(RuntimeError):
    pass


def read_ply(path, _fn="visma_io_read_ply"):
    """open3d::ReadPointCloudFromPLY / ReadTriangleMeshFromPLY -> dict(xyz, normals, colors, faces)."""
    L = load()
    L.visma_io_last_error.restype = C.c_char_p
    c = CIoCloud()
    rc = getattr(L, _fn)(str(path).encode(), C.byref(c))
    if rc != OK:
        raise IoError("%s: %s" % (_fn, L.visma_io_last_error().decode()))
    def take(ptr, n, cols, dt):
        if n == 0:
            return np.zeros((0, cols), dt)
        return np.ctypeslib.as_array(ptr, shape=(n * cols,)).astype(dt).reshape(n, cols).copy()
    out = dict(xyz=take(c.xyz, c.n, 3, np.float64), normals=take(c.normals, c.n_normals, 3, np.float64),
               colors=take(c.colors, c.n_colors, 3, np.float64), faces=take(c.faces, c.n_faces, 3, np.int32))
    L.visma_io_free_cloud(C.byref(c))
    return out


def read_pcd(path):
    """open3d::ReadPointCloudFromPCD -> dict(xyz, normals, colors, faces=empty)."""
    return read_ply(path, "visma_io_read_pcd")


class CIoPose(C.Structure):
    _fields_ = [("name", C.c_char * 256), ("id", C.c_int), ("status", C.c_int), ("T", C.c_double * 12)]


def _poses(fn, *args):
    L = load()
    L.visma_io_last_error.restype = C.c_char_p
    L.visma_io_free.argtypes = [C.c_void_p]
    ptr = C.POINTER(CIoPose)()
    n = C.c_int64(0)
    rc = getattr(L, fn)(*args, C.byref(ptr), C.byref(n))
    if rc != OK:
        raise IoError("%s: %s" % (fn, L.visma_io_last_error().decode()))
    out = [dict(name=ptr[i].name.decode(), id=ptr[i].id, status=ptr[i].status,
                T=np.array(list(ptr[i].T)).reshape(3, 4)) for i in range(n.value)]
    L.visma_io_free(ptr)
    return out


# ---- the gravity alignment and pose composition of feh::AnnotationTool (host arithmetic, no context) -------------
def find_plane_normal(xyz):
    """feh::FindPlaneNormal (include/geometry.h:18-26), with Eigen's sign of the singular vector."""
    xyz = _f64(xyz, (-1, 3)); out = np.empty(3)
    rc = load().visma_geom_find_plane_normal(_p(xyz, _dp), C.c_int64(len(xyz)), _p(out, _dp))
    if rc != OK:
        raise IcpError(rc, "visma_geom_find_plane_normal")
    return out


def jacobi_svd3(A):
    """Eigen::JacobiSVD<Matrix3d>(A, ComputeFullU | ComputeFullV) -> (U, S, V)."""
    A = _f64(A, (9,)); U = np.empty(9); S = np.empty(3); V = np.empty(9)
    rc = load().visma_geom_jacobi_svd3(_p(A, _dp), _p(U, _dp), _p(S, _dp), _p(V, _dp))
    if rc != OK:
        raise IcpError(rc, "visma_geom_jacobi_svd3")
    return U.reshape(3, 3), S, V.reshape(3, 3)


def rotation_between_vectors(u, v):
    """feh::RotationBetweenVectors (core/utils.h:229-233)."""
    u = _f64(u, (3,)); v = _f64(v, (3,)); R = np.empty(9)
    rc = load().visma_geom_rotation_between_vectors(_p(u, _dp), _p(v, _dp), _p(R, _dp))
    if rc != OK:
        raise IcpError(rc, "visma_geom_rotation_between_vectors")
    return R.reshape(3, 3)


def centre_on_floor(xyz):
    """(-mean_x, -min_y, -mean_z): the translation of T1 / T2 (src/annotation.cpp:114-119, 128-132)."""
    xyz = _f64(xyz, (-1, 3)); t = np.empty(3)
    rc = load().visma_geom_centre_on_floor(_p(xyz, _dp), C.c_int64(len(xyz)), _p(t, _dp))
    if rc != OK:
        raise IcpError(rc, "visma_geom_centre_on_floor")
    return t


def annot_total_pose(T0, T1, T2, T3):
    """Ttot = (T1 T0)^-1 T3 T2 (src/annotation.cpp:147-153)."""
    a = [_f64(T, (16,)) for T in (T0, T1, T2, T3)]; out = np.empty(16)
    rc = load().visma_annot_total_pose(*[_p(x, _dp) for x in a], _p(out, _dp))
    if rc != OK:
        raise IcpError(rc, "visma_annot_total_pose")
    return out.reshape(4, 4)


def read_alignment_json(path):
    """alignment.json (name -> 3x4 pose) -> list of dict(name, T), in key order like the reference's loop."""
    return _poses("visma_io_read_alignment_json", str(path).encode())


def read_result_json(path, packet=-1):
    """result.json -> the objects of one packet (default: the last): dict(id, status, name, T)."""
    return _poses("visma_io_read_result_json", str(path).encode(), C.c_int64(packet))


def write_alignment_json(path, poses):
    """poses: iterable of (name, 3x4 or 4x4 matrix)."""
    L = load()
    L.visma_io_last_error.restype = C.c_char_p
    poses = list(poses)
    arr = (CIoPose * max(len(poses), 1))()
    for i, (name, T) in enumerate(poses):
        arr[i].name = str(name).encode()
        T = np.asarray(T, np.float64)[:3, :4]
        arr[i].T = (C.c_double * 12)(*T.reshape(12))
    rc = L.visma_io_write_alignment_json(str(path).encode(), arr, C.c_int64(len(poses)))
    if rc != OK:
        raise IoError("visma_io_write_alignment_json: %s" % L.visma_io_last_error().decode())


def read_obj(path):
    """igl::readOBJ(path, V, F) -> (V [nv x 3], F [nf x face_size])."""
    L = load()
    L.visma_io_last_error.restype = C.c_char_p
    L.visma_io_free.argtypes = [C.c_void_p]
    V, F = _dp(), _ip()
    nv, nf, fs = C.c_int64(0), C.c_int64(0), C.c_int(0)
    rc = L.visma_io_read_obj(str(path).encode(), C.byref(V), C.byref(nv), C.byref(F), C.byref(nf), C.byref(fs))
    if rc != OK:
        raise IoError("visma_io_read_obj: %s" % L.visma_io_last_error().decode())
    v = np.ctypeslib.as_array(V, shape=(max(3 * nv.value, 1),))[:3 * nv.value].reshape(-1, 3).copy()
    f = np.ctypeslib.as_array(F, shape=(max(nf.value * fs.value, 1),))[:nf.value * fs.value].reshape(nf.value, max(fs.value, 0)).copy()
    L.visma_io_free(V); L.visma_io_free(F)
    return v, f


def tile_config():
    L = load()
    a = C.c_int(); b = C.c_int(); c = C.c_int()
    L.visma_icp_get_tile_config(C.byref(a), C.byref(b), C.byref(c))
    return {"s_tile": a.value, "t_chunk": b.value, "block": c.value}


def solve_from_stats(stats, solver=SOLVER_KABSCH, with_scaling=False):
    L = load()
    st = _f64(stats, (NSTATS,)); T = np.empty(16)
    rc = L.visma_icp_solve_from_stats(_p(st, _dp), int(solver), int(bool(with_scaling)), _p(T, _dp))
    if rc != OK:
        raise IcpError(rc, "solve_from_stats")
    return T.reshape(4, 4)


def solve_from_stats_axis(stats, axis, plane=False):
    """the update constrained to a rotation about `axis` plus a translation (visma_icp_solve_from_stats_axis): the closed
    form (plane=False) or one 4-unknown Gauss-Newton point-to-plane step (plane=True)"""
    L = load()
    st = _f64(stats, (NSTATS,)); a = _f64(axis, (3,)); T = np.empty(16)
    rc = L.visma_icp_solve_from_stats_axis(_p(st, _dp), int(bool(plane)), _p(a, _dp), _p(T, _dp))
    if rc != OK:
        raise IcpError(rc, "solve_from_stats_axis")
    return T.reshape(4, 4)
