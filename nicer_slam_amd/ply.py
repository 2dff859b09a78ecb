"""PLY files: ``read_ply`` (binary little-endian or ASCII, any scalar property types, polygons fan-triangulated), ``write_ply`` (the
binary layout of the meshes this package makes) and ``write_mesh_ply``, what the command lines of the mesh tools end with.  A leaf
module: it needs numpy and torch alone, so a mesh tool can read and write a file without importing the render stack.
``inference`` re-exports the first two under their old names.
"""
import numpy as np
import torch


def write_ply(path, mesh):
    """Binary little-endian PLY of a ``marching_cubes`` / ``extract_mesh`` dict: per vertex float x y z nx ny nz (+ uchar
    red green blue when ``colors`` is present, round(255 * clamp(c, 0, 1))), faces as a uchar-counted int32 list."""
    v = mesh["verts"].detach().cpu().numpy().astype("<f4")
    n = mesh["normals"].detach().cpu().numpy().astype("<f4")
    f = mesh["faces"].detach().cpu().numpy().astype("<i4")
    col = mesh.get("colors")
    vfields = [(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")]
    if col is not None:
        vfields += [(k, "u1") for k in ("red", "green", "blue")]
    vrec = np.empty(v.shape[0], dtype=vfields)
    for i, k in enumerate(("x", "y", "z")):
        vrec[k] = v[:, i]
        vrec["n" + k] = n[:, i]
    if col is not None:
        c = np.rint(np.clip(col.detach().float().cpu().numpy(), 0, 1) * 255).astype(np.uint8)
        for i, k in enumerate(("red", "green", "blue")):
            vrec[k] = c[:, i]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    head += [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")]
    if col is not None:
        head += [f"property uchar {k}" for k in ("red", "green", "blue")]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path):
    """Read a PLY mesh (binary little-endian or ASCII, any scalar property types): dict of numpy ``verts`` [V,3] float32,
    ``faces`` [F,3] int32 (polygons fan-triangulated: (v0, v_k, v_k+1)), plus ``normals`` [V,3] float32 when nx ny nz are present
    and ``colors`` [V,3] float32 in [0, 1] (uchar / 255, other types as stored) when red green blue are.  The file comes from
    outside the program: a malformed header, a truncated body or a face index outside [0, V) raises ValueError.  A ``write_ply``
    -> ``read_ply`` round trip is exact (colours as the written uchar / 255)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic or no end_header)")
    nl = data.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"{path}: header not terminated")
    try:
        header = data[:end].decode("ascii").splitlines()
    except UnicodeDecodeError as e:
        raise ValueError(f"{path}: header is not ASCII") from e
    body = data[nl + 1:]
    fmt, elements = None, []
    for line in header[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if len(tok) != 3 or tok[1] not in ("ascii", "binary_little_endian"):
                raise ValueError(f"{path}: unsupported format {line!r}")
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit():
                raise ValueError(f"{path}: bad element line {line!r}")
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if len(tok) == 5 and tok[1] == "list" and tok[2] in _PLY_TYPES and tok[3] in _PLY_TYPES:
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            elif len(tok) == 3 and tok[1] in _PLY_TYPES:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
            else:
                raise ValueError(f"{path}: bad property line {line!r}")
        else:
            raise ValueError(f"{path}: unknown header line {line!r}")
    if fmt is None:
        raise ValueError(f"{path}: no format line")
    out = {}
    if fmt == "ascii":
        words = body.split()
        pos = 0

        def take(k):
            nonlocal pos
            if pos + k > len(words):
                raise ValueError(f"{path}: truncated body")
            w = words[pos:pos + k]
            pos += k
            return w
    else:
        pos = 0
    for name, count, props in elements:
        has_list = any(p[2] is not None for p in props)
        fixed = None
        if fmt == "binary_little_endian" and len(props) == 1 and has_list and count > 0:
            _, t, it = props[0]                      # one list property: try a fixed length (triangle meshes)
            if pos + np.dtype(t).itemsize <= len(body):
                k = int(np.frombuffer(body, "<" + t, 1, pos)[0])
                fixed = np.dtype([("n", "<" + t), ("v", "<" + it, (k,))]) if k >= 0 else None
        if fixed is not None and pos + fixed.itemsize * count <= len(body) and \
                (np.frombuffer(body, fixed, count, pos)["n"] == fixed["v"].shape[0]).all():
            rec = np.frombuffer(body, fixed, count, pos)
            pos += fixed.itemsize * count
            cols = {props[0][0]: rec["v"].astype(np.int64)}
        elif fmt == "binary_little_endian" and not has_list:
            dt = np.dtype([(p[0], "<" + p[1]) for p in props])
            nbytes = dt.itemsize * count
            if pos + nbytes > len(body):
                raise ValueError(f"{path}: truncated body in element {name!r}")
            rec = np.frombuffer(body, dtype=dt, count=count, offset=pos)
            pos += nbytes
            cols = {p[0]: rec[p[0]] for p in props}
        else:
            cols = {p[0]: [] for p in props}
            for _ in range(count):
                for pname, t, it in props:
                    if fmt == "ascii":
                        if it is None:
                            cols[pname].append(np.array(take(1), dtype=np.float64 if t[0] == "f" else np.int64)[0])
                        else:
                            n = int(take(1)[0])
                            if n < 0:
                                raise ValueError(f"{path}: negative list length")
                            cols[pname].append(np.array(take(n), dtype=np.int64))
                    else:
                        if it is None:
                            sz = np.dtype(t).itemsize
                            if pos + sz > len(body):
                                raise ValueError(f"{path}: truncated body in element {name!r}")
                            cols[pname].append(np.frombuffer(body, "<" + t, 1, pos)[0])
                            pos += sz
                        else:
                            sz = np.dtype(t).itemsize
                            if pos + sz > len(body):
                                raise ValueError(f"{path}: truncated body in element {name!r}")
                            n = int(np.frombuffer(body, "<" + t, 1, pos)[0])
                            pos += sz
                            isz = np.dtype(it).itemsize
                            if n < 0 or pos + n * isz > len(body):
                                raise ValueError(f"{path}: truncated body in element {name!r}")
                            cols[pname].append(np.frombuffer(body, "<" + it, n, pos).astype(np.int64))
                            pos += n * isz
            for pname, t, it in props:
                if it is None:
                    cols[pname] = np.asarray(cols[pname], dtype=t)
        out[name] = (count, cols)
    if "vertex" not in out:
        raise ValueError(f"{path}: no vertex element")
    V, vc = out["vertex"]
    if not all(k in vc for k in ("x", "y", "z")):
        raise ValueError(f"{path}: vertex element without x y z")
    mesh = {"verts": np.stack([np.asarray(vc[k]).astype(np.float32) for k in ("x", "y", "z")], -1).reshape(V, 3)}
    if all(k in vc for k in ("nx", "ny", "nz")):
        mesh["normals"] = np.stack([np.asarray(vc[k]).astype(np.float32) for k in ("nx", "ny", "nz")], -1).reshape(V, 3)
    if all(k in vc for k in ("red", "green", "blue")):
        c = np.stack([np.asarray(vc[k]) for k in ("red", "green", "blue")], -1).reshape(V, 3)
        mesh["colors"] = c.astype(np.float32) / 255.0 if c.dtype == np.uint8 else c.astype(np.float32)
    tris = []
    if "face" in out:
        F, fc = out["face"]
        lists = fc.get("vertex_indices", fc.get("vertex_index"))
        if lists is None:
            raise ValueError(f"{path}: face element without vertex_indices")
        if isinstance(lists, np.ndarray) and lists.ndim == 2 and lists.shape[1] >= 3:
            if lists.size and (lists.min() < 0 or lists.max() >= V):
                raise ValueError(f"{path}: face index outside [0, {V})")
            k = lists.shape[1]
            fan = [np.stack([lists[:, 0], lists[:, j], lists[:, j + 1]], -1) for j in range(1, k - 1)]
            mesh["faces"] = np.stack(fan, 1).reshape(-1, 3).astype(np.int32)
            return mesh
        for poly in lists:
            poly = np.asarray(poly, dtype=np.int64)
            if poly.size < 3:
                raise ValueError(f"{path}: face with fewer than 3 vertices")
            if poly.min() < 0 or poly.max() >= V:
                raise ValueError(f"{path}: face index outside [0, {V})")
            for k in range(1, poly.size - 1):
                tris.append((poly[0], poly[k], poly[k + 1]))
    mesh["faces"] = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    return mesh


def write_mesh_ply(path, mesh):
    """``write_ply`` for a mesh dict of arrays or tensors as the mesh tools return it: ``verts``, ``faces``, ``normals`` and ``colors``
    are kept, every other key is dropped; ``write_ply`` stores normals, so a mesh without them gets zeros."""
    out = {k: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
           for k, x in mesh.items() if k in ("verts", "faces", "normals", "colors")}
    if "normals" not in out:
        out["normals"] = torch.zeros_like(out["verts"])
    write_ply(path, out)
