"""The shared argument checks of nicer_slam_amd/mesh_args.py held to their contract directly, without a GPU: every count bound at its
edge (on expanded tensors: nothing that size is allocated), the int32 range, dtypes and shapes, numpy against torch, the restorer,
and ValueError for a malformed argument before RuntimeError for a missing GPU."""
import numpy as np
import pytest
import torch

from nicer_slam_amd import mesh_args as A


@pytest.fixture
def no_gpu(monkeypatch):
    """the state of a machine without a GPU, wherever the test runs: what need_gpu asks says no"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


TRI = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
VERTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)


def many_faces(F, dtype=torch.int32):
    return torch.zeros(1, 3, dtype=dtype).expand(F, 3)


def test_the_three_bounds_are_what_the_kernels_index():
    assert A.MAX_FACES == 2 ** 31 - 1
    assert 3 * A.MAX_FACES_EDGES < 2 ** 31 <= 3 * (A.MAX_FACES_EDGES + 1)
    assert 6 * A.MAX_FACES_RINGS < 2 ** 31 <= 6 * (A.MAX_FACES_RINGS + 1)


@pytest.mark.parametrize("bound", [A.MAX_FACES, A.MAX_FACES_EDGES, A.MAX_FACES_RINGS])
def test_face_count_at_the_bound_passes_and_one_more_raises(bound, no_gpu):
    f = A.checked_faces(many_faces(bound), "t", max_faces=bound)
    assert f.shape == (bound, 3) and f.dtype == torch.int32
    with pytest.raises(ValueError, match="^t: count out of range"):
        A.checked_faces(many_faces(bound + 1), "t", max_faces=bound)
    with pytest.raises(RuntimeError, match="^t: needs a GPU"):  # well-formed at the bound: the next thing missing is the GPU
        A.cuda_faces(many_faces(bound), 1, None, "t", max_faces=bound)
    with pytest.raises(ValueError):                            # malformed: refused before the GPU is asked for
        A.cuda_faces(many_faces(bound + 1), 1, None, "t", max_faces=bound)


@pytest.mark.parametrize("n_verts", [-1, 2 ** 31])
def test_vertex_count_out_of_range_raises(n_verts):
    with pytest.raises(ValueError, match="count out of range"):
        A.checked_faces(TRI, "t", n_verts=n_verts)
    assert A.checked_faces(TRI, "t", n_verts=2 ** 31 - 1).shape == (2, 3)


@pytest.mark.parametrize("bad", [2 ** 31, -2 ** 31 - 1])
def test_int64_index_outside_int32_raises(bad):
    f = np.array([[0, 1, bad]], np.int64)
    for x in (f, torch.from_numpy(f)):
        with pytest.raises(ValueError, match="^t: face index outside int32"):
            A.checked_faces(x, "t")
    edge = np.array([[-2 ** 31, 0, 2 ** 31 - 1]], np.int64)    # the extremes of int32 themselves pass
    assert A.checked_faces(edge, "t").dtype == torch.int64


def test_int32_faces_are_never_read_back():
    class NoReadBack(torch.Tensor):
        @classmethod
        def __torch_function__(cls, func, types, args=(), kwargs=None):
            assert func.__name__ not in ("min", "max", "amin", "amax", "aminmax"), "the range check read int32 faces"
            return super().__torch_function__(func, types, args, kwargs or {})
    A.checked_faces(torch.from_numpy(TRI).as_subclass(NoReadBack), "t")
    with pytest.raises(AssertionError):                        # the probe sees the read of an int64 list
        A.checked_faces(torch.from_numpy(TRI).long().as_subclass(NoReadBack), "t")


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16, np.uint8])
def test_faces_of_another_dtype_raise(dtype):
    with pytest.raises(ValueError, match="^t: faces must be int32 or int64"):
        A.checked_faces(TRI.astype(dtype), "t")
    assert A.checked_faces(TRI.astype(np.int16), "t", dtypes=None).dtype == torch.int16     # (mesh_eval's indexes take any)


@pytest.mark.parametrize("shape", [(2, 2), (6,), (1, 2, 3), (2, 4)])
def test_faces_of_another_shape_raise(shape):
    with pytest.raises(ValueError, match=r"^t: faces must be \[F, 3\]"):
        A.checked_faces(np.zeros(shape, np.int32), "t")


def test_require_cuda_refuses_host_faces():
    for x in (TRI, torch.from_numpy(TRI)):
        with pytest.raises(ValueError, match="^t: faces must be a CUDA tensor"):
            A.checked_faces(x, "t", require_cuda=True)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_numpy_and_torch_faces_give_equal_results(dtype):
    a = A.checked_faces(TRI.astype(dtype), "t", n_verts=4)
    b = A.checked_faces(torch.from_numpy(TRI.astype(dtype)), "t", n_verts=4)
    assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
    empty = A.checked_faces(np.zeros((0, 3), dtype), "t")
    assert empty.shape == (0, 3)


def test_as_tensor_shares_memory_with_a_contiguous_array():
    a = TRI.copy()
    t = A.as_tensor(a)
    t[0, 0] = 7
    assert a[0, 0] == 7
    assert torch.equal(A.as_tensor(TRI[:, ::-1]), torch.from_numpy(TRI[:, ::-1].copy()))
    assert A.as_tensor(t) is t


def test_mask_length_is_checked_before_the_gpu():
    with pytest.raises(ValueError, match="^t: mask of 3 for 2 faces"):
        A.cuda_faces(TRI, 4, np.ones(3, bool), "t")


def mesh(**over):
    m = {"verts": VERTS, "faces": TRI, "normals": np.zeros((4, 3), np.float32), "colors": np.ones((4, 3), np.float32)}
    m.update(over)
    return {k: x for k, x in m.items() if x is not ...}


@pytest.mark.parametrize("bad", [
    mesh(verts=...), mesh(faces=...), [VERTS, TRI],                                        # a missing key, not a dict
    mesh(verts=VERTS[:, :2]), mesh(verts=VERTS.reshape(-1)), mesh(verts=VERTS.reshape(2, 2, 3)),   # verts not [V, 3]
    mesh(colors=np.ones((3, 3), np.float32)), mesh(normals=np.zeros((3, 3), np.float32)),  # an attribute with V - 1 rows
    mesh(colors=np.ones((4, 4), np.float32)),                                              # ... and one that is not three wide
    mesh(verts=VERTS.astype(np.int32)), mesh(verts=torch.from_numpy(VERTS).long()),        # integer verts under float_verts
    mesh(faces=TRI.astype(np.float32)), mesh(faces=TRI[:, :2]), mesh(faces=np.array([[0, 1, 2 ** 31]])),
], ids=lambda m: "mesh")
def test_checked_mesh_refuses_before_the_gpu(bad):
    with pytest.raises(ValueError, match="^t: "):
        A.checked_mesh(bad, "t", float_verts=True, attributes=("normals", "colors"))


def test_checked_mesh_options_are_options(no_gpu):
    ints = mesh(verts=VERTS.astype(np.int32), colors=np.ones((4, 3), np.uint8))
    with pytest.raises(RuntimeError, match="^t: needs a GPU"):                  # integer verts and colours pass without the flags
        A.checked_mesh(ints, "t", attributes=("colors",))
    with pytest.raises(ValueError, match="colors must be floating point"):
        A.checked_mesh(ints, "t", attributes=("colors",), float_attributes=True)
    with pytest.raises(RuntimeError):                                           # an attribute that is not listed is not looked at
        A.checked_mesh(mesh(colors=np.ones((3, 3), np.float32)), "t", attributes=("normals",))
    with pytest.raises(RuntimeError):                                           # None is "absent"
        A.checked_mesh(mesh(colors=None), "t", attributes=("colors",))
    with pytest.raises(ValueError, match="count out of range"):                 # the face bound is the caller's
        A.checked_mesh(mesh(), "t", max_faces=1)


def test_checked_rows_counts_rows_only():
    A.checked_rows(mesh(colors=np.ones((4, 7))), 4, "t")
    with pytest.raises(ValueError, match="^t: 'colors' has 3 rows for 4 vertices"):
        A.checked_rows(mesh(colors=np.ones((3, 7))), 4, "t")


def test_mesh_dict_tensors_keeps_dtypes_and_carries_the_rest():
    m, was_numpy, orig = A.mesh_dict_tensors(mesh(verts=VERTS.astype(np.float64), note="kept"))
    assert was_numpy and orig is None and m["note"] == "kept"
    assert m["verts"].dtype == torch.float64 and m["faces"].dtype == torch.int32 and m["colors"].dtype == torch.float32
    t = {k: torch.from_numpy(x) for k, x in mesh().items()}
    m, was_numpy, orig = A.mesh_dict_tensors(t)
    assert not was_numpy and orig == torch.device("cpu") and all(m[k] is t[k] for k in t)
    for bad in (mesh(verts=...), mesh(verts=VERTS[:, :2]), mesh(faces=TRI[:, :2]), mesh(normals=np.zeros((3, 3), np.float32))):
        with pytest.raises(ValueError, match="^mesh: "):
            A.mesh_dict_tensors(bad)


def test_the_restorer_gives_the_callers_kind_back():
    r = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    back = A.restorer(*A.kind(TRI))(r)
    assert isinstance(back, np.ndarray) and back.dtype == np.int32 and (back == r.numpy()).all()
    src = torch.from_numpy(TRI)
    back = A.restorer(*A.kind(src))(r)
    assert torch.is_tensor(back) and back.device == src.device and torch.equal(back, r)
    d = A.restore_dict({"a": r, "n": 3, "s": "x"}, True, None)
    assert isinstance(d["a"], np.ndarray) and d["n"] == 3 and d["s"] == "x"
    assert A.kind(TRI) == (True, None) and A.kind(src) == (False, torch.device("cpu"))


def test_ptr_is_null_for_nothing():
    assert A.ptr(None) is None and A.ptr(torch.empty(0, 3)) is None
    t = torch.zeros(2, 3)
    assert A.ptr(t) == t.data_ptr() != 0
    assert A.workspace(0, "cpu").numel() == 0 and A.workspace(5, "cpu").dtype == torch.uint8


def test_points_must_be_cuda_tensors():
    for x in (VERTS, torch.from_numpy(VERTS)):
        with pytest.raises(ValueError, match="^t: needs a CUDA tensor"):
            A.checked_points(x, "t")


def test_value_error_comes_before_the_missing_gpu(no_gpu):
    with pytest.raises(RuntimeError, match="^t: needs a GPU"):
        A.need_gpu("t")
    for call in (lambda: A.to_cuda(TRI, "t"), lambda: A.to_cuda(torch.from_numpy(TRI), "t"), lambda: A.cuda_faces(TRI, 4, None, "t"),
                 lambda: A.cuda_faces(TRI, 4, np.ones(2, bool), "t"), lambda: A.checked_mesh(mesh(), "t", float_verts=True)):
        with pytest.raises(RuntimeError):
            call()
    for call in (lambda: A.cuda_faces(TRI.astype(np.float32), 4, None, "t"), lambda: A.cuda_faces(TRI, -1, None, "t"),
                 lambda: A.checked_mesh(mesh(verts=VERTS[:3]), "t", attributes=("colors",))):
        with pytest.raises(ValueError):
            call()
