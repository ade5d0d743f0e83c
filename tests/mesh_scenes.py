"""Generated scenes of the mesh render tests (numpy only): the open tube of tests/test_template_gpu.py, restated, under
an orbit camera, and the hand-placed clip-space triangles that exercise the rasterizer's edge cases."""
import numpy as np


def tube(nu=24, nv=12, r=0.3, h=1.0):
    """(vertices float32 [V,3], triangles int32 [2 nu nv, 3], vertex normals float32 [V,3]) of an open tube around z."""
    ang = 2.0 * np.pi * np.arange(nu) / nu
    v = np.array([[r * np.cos(a), r * np.sin(a), h * j / nv] for j in range(nv + 1) for a in ang], dtype=np.float64)
    quads = np.array([[j * nu + i, j * nu + (i + 1) % nu, (j + 1) * nu + (i + 1) % nu, (j + 1) * nu + i]
                      for j in range(nv) for i in range(nu)], dtype=np.int64)
    tri = np.concatenate((quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]))
    vn = np.array([[np.cos(a), np.sin(a), 0.0] for _ in range(nv + 1) for a in ang], dtype=np.float64)
    return v.astype(np.float32), tri.astype(np.int32), vn.astype(np.float32)


def look_at_pose(campos, target=(0.0, 0.0, 0.5), up=(0.0, 0.0, 1.0)):
    """Camera-to-world matrix [4,4] of an OpenGL camera (looks along -z, y up) at ``campos``."""
    campos, target, up = (np.asarray(a, dtype=np.float64) for a in (campos, target, up))
    z = campos - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, campos
    return pose.astype(np.float32)


def perspective(fovy, near=0.01, far=100):
    """The reference's netf/view_core/camera.py:perspective, restated (the package's copy is checked against values)."""
    y = np.tan(fovy / 2)
    return np.array([[1 / y, 0, 0, 0], [0, -1 / y, 0, 0],
                     [0, 0, -(far + near) / (far - near), -(2 * far * near) / (far - near)], [0, 0, -1, 0]], dtype=np.float32)


# above the rim, so that the inside of the far wall shows through the open top behind the near wall
CAMPOS = (1.5, 0.4, 1.45)
FOVY = 0.75


def clip_positions(v, pose, proj):
    """float32 [V,4]: the renderer's v_cam @ proj.T, in float32 numpy."""
    vh = np.concatenate((v, np.ones((v.shape[0], 1), np.float32)), axis=1).astype(np.float32)
    v_cam = (vh @ np.linalg.inv(pose).T.astype(np.float32)).astype(np.float32)
    return (v_cam @ proj.T).astype(np.float32), v_cam


def tube_clip(nu=24, nv=12):
    v, tri, vn = tube(nu, nv)
    pos, _ = clip_positions(v, look_at_pose(CAMPOS), perspective(FOVY))
    return pos, tri


EXTRA = {   # name -> clip-space corners (x, y, z, w); the tube's z/w lies around 0.99
    "large_a": [(-0.95, -0.9, 0.980, 1), (0.95, -0.8, 0.9995, 1), (-0.1, 0.95, 0.990, 1)],      # viewport-sized and
    "large_b": [(-0.9, -0.85, 0.9995, 1), (0.9, -0.95, 0.980, 1), (0.1, 0.9, 0.990, 1)],        # interpenetrating
    "dup_0": [(-0.9, 0.5, 0.5, 1), (-0.55, 0.55, 0.5, 1), (-0.7, 0.9, 0.5, 1)],
    "dup_1": None,                                                                              # same corners as dup_0
    "zero_area": [(0.5, 0.5, 0.3, 1), (0.6, 0.6, 0.3, 1), (0.7, 0.7, 0.3, 1)],
    "behind": [(0.2, -0.6, 0.4, 1), (0.5, -0.6, 0.4, 1), (0.3, -0.2, 0.4, -0.5)],               # a vertex at w <= 0
    "w_zero": [(0.2, -0.6, 0.4, 1), (0.5, -0.6, 0.4, 1), (0.3, -0.2, 0.4, 0.0)],
    "partly_out": [(0.7, -0.9, 0.45, 1), (1.6, -0.7, 0.45, 1), (0.8, -0.3, 0.45, 1)],
    "wholly_out": [(1.2, 0.1, 0.4, 1), (1.7, 0.2, 0.4, 1), (1.4, 0.6, 0.4, 1)],
    "z_range": [(-0.9, -0.1, 0.6, 1), (-0.5, -0.15, 1.6, 1), (-0.7, 0.3, 0.8, 1)],              # z/w > 1 over a part
    "w_varies": [(0.9, 0.8, 0.6, 2.0), (1.5, 1.1, 0.7, 2.0), (0.8, 1.6, 0.5, 2.5)],             # perspective u, v
}


def edge_case_scene():
    """(pos float32 [V,4], tri int32 [F,3], names): the 576-triangle tube plus the EXTRA triangles; ``names[i]`` is the
    index of extra triangle i."""
    pos, tri = tube_clip()
    verts, tris, names = [pos], [tri], {}
    base = pos.shape[0]
    for name, corners in EXTRA.items():
        names[name] = sum(t.shape[0] for t in tris)
        if corners is None:
            tris.append(tris[-1].copy())
            continue
        verts.append(np.asarray(corners, dtype=np.float32))
        tris.append(np.array([[base, base + 1, base + 2]], dtype=np.int32))
        base += 3
    return np.concatenate(verts).astype(np.float32), np.concatenate(tris).astype(np.int32), names
