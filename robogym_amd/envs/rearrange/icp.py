"""Host side of GoalArgs.rot_dist_type "icp" (goals/object_state.py:128-149, 258-290; utils/icp.py): the objects' point clouds, made once from the compiled model, and a
float64 restatement of the reference's ICP rotation distance, which the device kernel (robogym_amd/csrc/ra_icp_kernel.h) is tested against.

`object_point_clouds` follows get_all_vertices (common/utils.py:294-340): every geom's vertices through the geom's pose into the body frame.  The SOURCE cloud of an object
is its raw vertex list (current_state["vertices"]), cut to `icp_max_num_vertices`; the TARGET cloud is the same vertices with the mesh subdivided
(get_target_vertices(subdivide_threshold=2 * icp_error_threshold)).  Two stated deviations:
  * the reference draws a new random subset of the source at every call from a generator that runs on; here the subset is fixed, the first `icp_max_num_vertices`
    entries of RandomState(0).permutation(n) -- the reference's first draw;
  * the compiled models hold each convex part's hull vertices and no faces: the faces are each part's hull triangles (scipy.spatial.ConvexHull) and the subdivision is
    restated (every triangle with an edge longer than max_edge is split in four at its edge midpoints until none is left; duplicate points merged), so the target cloud
    covers the same surface to the same edge bound but is not trimesh.remesh.subdivide_to_size's vertex list.
"""
import numpy as np

#: the kernel's capacity for source points per object (ra_icp_kernel.h RA_ICP_MAXSRC: two per thread of a 256-thread workgroup)
ICP_MAX_SOURCE_POINTS = 512
ICP_DEFAULT_ANGLE = np.pi / 2      # the "arbitrarily large" rotation distance of a refused fit (object_state.py:273-274), per Euler angle


def _quat2mat(q):
    w, x, y, z = (float(v) for v in q)
    n = w * w + x * x + y * y + z * z
    s = 2.0 / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                     [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                     [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]])


def mat2euler(M):
    """rotation.mat2euler (robogym/utils/rotation.py) of one 3 x 3 matrix, float64"""
    M = np.asarray(M, dtype=np.float64)
    cy = np.sqrt(M[2, 2] * M[2, 2] + M[1, 2] * M[1, 2])
    if cy > 4.0 * np.finfo(np.float64).eps:
        return np.array([-np.arctan2(M[1, 2], M[2, 2]), -np.arctan2(-M[0, 2], cy), -np.arctan2(M[0, 1], M[0, 0])])
    return np.array([0.0, -np.arctan2(-M[0, 2], cy), -np.arctan2(-M[1, 0], M[1, 1])])


def half_extent_norm(points):
    """norm of the half extents of the points' axis-aligned box (utils/mesh.py get_vertices_bounding_box()[-1])"""
    points = np.asarray(points)
    return float(np.linalg.norm((points.max(0) - points.min(0)) / 2.0))


def subdivide_to_edge(verts, faces, max_edge):
    """Every triangle with an edge longer than `max_edge` split in four at its edge midpoints, repeated until none is left; returns the points (duplicates merged, first
    occurrence kept).  A midpoint shared by two triangles of one round is made once."""
    verts = [np.asarray(v, dtype=np.float64) for v in np.asarray(verts, dtype=np.float64)]
    faces = [tuple(int(i) for i in f) for f in np.asarray(faces)]
    assert max_edge > 0
    while True:
        V = np.array(verts)
        F = np.array(faces, dtype=np.int64).reshape(-1, 3)
        edge = np.stack([np.linalg.norm(V[F[:, a]] - V[F[:, b]], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))], 1)
        split = edge.max(1) > max_edge
        if not split.any():
            break
        mid, out = {}, [f for f, s in zip(faces, split) if not s]

        def midpoint(i, j):
            key = (i, j) if i < j else (j, i)
            if key not in mid:
                mid[key] = len(verts)
                verts.append(0.5 * (verts[i] + verts[j]))
            return mid[key]

        for (a, b, c), s in zip(faces, split):
            if s:
                ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
                out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = out
    V = np.array(verts)
    _, first = np.unique(V, axis=0, return_index=True)
    return V[np.sort(first)], np.array(faces, dtype=np.int64).reshape(-1, 3), V


def body_geom_vertices(model, body):
    """Per geom of the body, in geom order: (vertices in the body frame [n, 3], is_mesh) -- get_geom_vertices through the geom's pose (common/utils.py:311-325)."""
    from robogym_amd.mujoco.mjcf_compiler import GEOM_BOX, GEOM_MESH, q2mat

    A = model.arrays
    out = []
    for g in np.nonzero(np.asarray(A["geom_bodyid"]) == body)[0]:
        R, p = q2mat(A["geom_quat"][g]), np.asarray(A["geom_pos"][g], dtype=np.float64)
        if A["geom_type"][g] == GEOM_MESH:
            m = int(A["geom_dataid"][g])
            adr, num = int(A["mesh_vertadr"][m]), int(A["mesh_vertnum"][m])
            v = np.asarray(A["mesh_vert"], dtype=np.float64).reshape(-1, 3)[adr:adr + num]
        elif A["geom_type"][g] == GEOM_BOX:
            s_ = A["geom_size"][g]      # (the corner order of get_geom_vertices: itertools.product([dx, -dx], [dy, -dy], [dz, -dz]))
            v = np.array([[sx * s_[0], sy * s_[1], sz * s_[2]] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=np.float64)
        else:
            raise NotImplementedError("icp point cloud of geom type %d (box and mesh geoms are built)" % A["geom_type"][g])
        out.append((v @ R.T + p, bool(A["geom_type"][g] == GEOM_MESH)))
    if not out:
        raise ValueError("body %d has no geoms" % body)
    return out


def subdivided_mesh_of_body(model, body, icp_error_threshold=0.15):
    """The body's subdivided surface as (points [pt, 3] with duplicates merged, faces [f, 3] into `vertices`, vertices [v, 3], max_edge), or None when a geom of the
    body is no mesh (the reference's faces are None for a box: no subdivision, common/utils.py:327).  max_edge = |half extents of the body's vertices| x 2 x threshold."""
    parts = body_geom_vertices(model, body)
    if not all(is_mesh for _, is_mesh in parts):
        return None
    from scipy.spatial import ConvexHull      # (imported locally, as the mesh processing of the model compiler does)

    raw = np.concatenate([v for v, _ in parts], 0)
    faces, off = [], 0
    for v, _ in parts:
        faces.append(ConvexHull(v).simplices.astype(np.int64) + off)
        off += len(v)
    max_edge = half_extent_norm(raw) * 2.0 * icp_error_threshold
    return subdivide_to_edge(raw, np.concatenate(faces, 0), max_edge) + (max_edge,)


def object_clouds_of_body(model, body, icp_error_threshold=0.15, icp_max_num_vertices=500):
    """(source [ps, 3], target [pt, 3], raw vertices [n, 3]) of one body, float64, in the body frame."""
    raw = np.concatenate([v for v, _ in body_geom_vertices(model, body)], 0)
    src = raw
    if len(raw) > icp_max_num_vertices:
        src = raw[np.random.RandomState(0).permutation(len(raw))[:icp_max_num_vertices]]
    mesh = subdivided_mesh_of_body(model, body, icp_error_threshold)
    return src, (raw.copy() if mesh is None else mesh[0]), raw


def object_point_clouds(model, num_objects, icp_error_threshold=0.15, icp_max_num_vertices=500):
    """The five arrays the kernel takes, float32 / int32, all points in the object's body frame:
    (src [N, Ps, 3] zero-padded, src_num [N], tgt [sum Pt, 3] flat, tgt_adr [N], tgt_num [N])."""
    if not 1 <= int(icp_max_num_vertices) <= ICP_MAX_SOURCE_POINTS:
        raise NotImplementedError("icp_max_num_vertices=%r: the ICP kernel holds at most %d source points per object (1..%d)" % (icp_max_num_vertices, ICP_MAX_SOURCE_POINTS, ICP_MAX_SOURCE_POINTS))
    if not float(icp_error_threshold) > 0:
        raise ValueError("icp_error_threshold must be positive, got %r" % (icp_error_threshold,))
    clouds = [object_clouds_of_body(model, model.name2id("body", "object%d" % i), float(icp_error_threshold), int(icp_max_num_vertices)) for i in range(num_objects)]
    ps = max(len(c[0]) for c in clouds)
    src = np.zeros((num_objects, ps, 3), dtype=np.float32)
    for i, c in enumerate(clouds):
        src[i, :len(c[0])] = c[0]
    src_num = np.array([len(c[0]) for c in clouds], dtype=np.int32)
    tgt_num = np.array([len(c[1]) for c in clouds], dtype=np.int32)
    tgt_adr = np.concatenate([[0], np.cumsum(tgt_num)[:-1]]).astype(np.int32)
    tgt = np.concatenate([c[1] for c in clouds], 0).astype(np.float32)
    return src, src_num, tgt, tgt_adr, tgt_num


def _nearest(src, tgt):
    """brute force: per source point the distance to and the index of its nearest target point; the lowest index among equal distances"""
    d2 = ((src[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)
    idx = np.argmin(d2, axis=1)
    return np.sqrt(d2[np.arange(len(src)), idx]), idx


def _best_fit(A, B):
    """least-squares rigid fit A -> B by centroids and the SVD of the 3 x 3 cross-covariance; a reflection is undone on the last row of Vt.  Returns (R, t)."""
    ca, cb = A.mean(0), B.mean(0)
    H = (A - ca).T @ (B - cb)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt = Vt.copy()
        Vt[2, :] *= -1
        R = Vt.T @ U.T
    return R, cb - R @ ca


def icp_rotation(src_world, tgt_world, error_threshold, max_iterations=5, tolerance=1e-6, dtype=np.float64, return_error=False):
    """The reference's ICP (utils/icp.py) restated: up to `max_iterations` rounds of nearest neighbours + best fit, stopped early when the mean neighbour distance moves
    by less than `tolerance`; one final fit from the original source to the moved one; accepted when the LAST round's largest neighbour distance is below
    `error_threshold` x the norm of the target cloud's half extents.  Returns R.T (the matrix whose mat2euler the reference takes) or None; with `return_error` also
    max_error / threshold.  `dtype=np.float32` runs the same code in single precision (for the spread measurement of tools/gen_golden_rearrange_icp.py only)."""
    A = np.asarray(src_world, dtype=dtype)
    B = np.asarray(tgt_world, dtype=dtype)
    src = A.copy()
    prev, max_error = dtype(0), dtype(0)
    for _ in range(max_iterations):
        dist, idx = _nearest(src, B)
        R, t = _best_fit(src, B[idx])
        src = (src @ R.T + t).astype(dtype)
        mean, max_error = dist.mean(), dist.max()
        if abs(prev - mean) < tolerance:
            break
        prev = mean
    R, _ = _best_fit(A, src)
    thr = dtype(error_threshold) * dtype(np.linalg.norm((B.max(0) - B.min(0)) / dtype(2)))
    out = R.T.copy() if max_error < thr else None
    return (out, float(max_error) / float(thr)) if return_error else out


def icp_euler_angle_difference(obj_quat, goal_quat, clouds, icp_error_threshold=0.15, dtype=np.float64):
    """_icp_euler_angle_difference (goals/object_state.py:258-290) for one env: `obj_quat`, `goal_quat` [N, 4] (w x y z) are the bodies' world rotations, `clouds` what
    `object_point_clouds` returned.  Object i's source cloud turned by its rotation against object i's target cloud turned by the goal's (neither translated); the Euler
    angles of the fit, or (pi/2, pi/2, pi/2) where it is refused.  Returns [N, 3] (before normalize_angles)."""
    src, src_num, tgt, tgt_adr, tgt_num = clouds
    out = np.full((len(obj_quat), 3), ICP_DEFAULT_ANGLE)
    for i in range(len(obj_quat)):
        s = np.asarray(src[i, :src_num[i]], dtype=np.float64) @ _quat2mat(obj_quat[i]).T
        t = np.asarray(tgt[tgt_adr[i]:tgt_adr[i] + tgt_num[i]], dtype=np.float64) @ _quat2mat(goal_quat[i]).T
        M = icp_rotation(s, t, icp_error_threshold, dtype=dtype)
        if M is not None:
            out[i] = mat2euler(M)
    return out
