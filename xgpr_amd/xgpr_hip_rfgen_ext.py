"""Operator surface of the reference's GPU extension module, served by libxgpr_hip.so.

Mirrors ``xGPR.xgpr_cuda_rfgen_cpp_ext`` (reference:
src/xGPR/random_feature_generation/gpu_rf_gen/xgpr_cuda_rfgen_cpp_ext.cpp:20-93): same
function names (``cuda*`` kept as aliases of the ``hip*`` names), same keyword names, same
in-place semantics, same error behaviour -- arguments are *not* converted (wrong dtype,
device or contiguity raises ``TypeError`` like nanobind's ``.noconvert()``), validation
failures raise ``RuntimeError`` with the reference's messages, and every function returns 0.

Arrays are device arrays of any producer that speaks DLPack (``__dlpack__`` / a DLPack capsule; a torch-ROCm
tensor exports device type kDLROCM) or ``__cuda_array_interface__`` -- what nanobind's
``nb::ndarray<..., nb::device::cuda>`` accepts in the reference, so its cupy callers
(kernels/basic_kernels/sorf_kernel_baseclass.py:104-126) can pass their arrays as they are.  They are adopted
zero-copy (``torch.from_dlpack`` / ``torch.as_tensor``): the in-place operators write the producer's own memory.
``seqlengths`` stays on the HOST (int32 numpy array or CPU tensor), as in the reference's CUDA module
(gpu_rf_gen/convolution_ops/rbf_convolution.h:19).  Calls are asynchronous on torch's current stream.
"""
import ctypes as C
import functools
import inspect

import numpy as np
import torch

from . import _lib

_LIB = _lib.load()

_T2S = {torch.float32: "f32", torch.float64: "f64"}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _adopt(obj, name):
    """A zero-copy torch view of a device array from any producer; never a conversion (a host array stays a host
    array and is then refused by _dev, like nanobind's .noconvert())."""
    if isinstance(obj, torch.Tensor) or obj is None:
        return obj
    try:
        if hasattr(obj, "__dlpack__") or type(obj).__name__ == "PyCapsule":
            return torch.from_dlpack(obj)
        if hasattr(obj, "__cuda_array_interface__"):
            return torch.as_tensor(obj, device="cuda")
    except (RuntimeError, ValueError, BufferError) as exc:
        raise TypeError(f"{name}: could not adopt the array through DLPack / __cuda_array_interface__: {exc}") from exc
    raise TypeError(f"{name}: expected a device array (torch tensor, DLPack or __cuda_array_interface__ producer)")


def _array_args(*names):
    """Decorator: the named arguments may come from any DLPack / __cuda_array_interface__ producer."""
    def wrap(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def inner(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            for nm in names:
                if nm in bound.arguments:
                    bound.arguments[nm] = _adopt(bound.arguments[nm], nm)
            return fn(*bound.args, **bound.kwargs)
        return inner
    return wrap


def _dev(t, name, dtype, ndim):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a device array")
    if not t.is_cuda:
        raise TypeError(f"{name}: expected a device tensor, got a host tensor")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.dim() != ndim:
        raise TypeError(f"{name}: expected {ndim} dims, got {t.dim()}")
    if not t.is_contiguous():
        raise TypeError(f"{name}: expected a C-contiguous array")
    return C.c_void_p(t.data_ptr())


def _ftype(t, name):
    if not isinstance(t, torch.Tensor) or t.dtype not in _T2S:
        raise TypeError(f"{name}: expected a float32 or float64 torch tensor")
    return _T2S[t.dtype]


def _workspace(nbytes, device):
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return ws, C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel())


def _sorf_ws(radem, width, inputArr):
    nbytes = _LIB.xgpr_sorf_workspace_bytes(radem.shape[2], int(width), inputArr.element_size())
    return _workspace(nbytes, inputArr.device)


def _conv_ws(radem, width, inputArr):
    """Workspace of a convolution operator call, with room for the longest-first processing order."""
    nbytes = _LIB.xgpr_conv_workspace_bytes(radem.shape[2], int(width), inputArr.element_size(), inputArr.shape[0])
    return _workspace(nbytes, inputArr.device)


def _seqlens(seqlengths, device):
    """Host int32 array (validated by the library on the host) + its device copy."""
    if isinstance(seqlengths, torch.Tensor):
        if seqlengths.is_cuda or seqlengths.dtype != torch.int32 or seqlengths.dim() != 1:
            raise TypeError("seqlengths: expected a 1-d int32 array on the host")
        host = seqlengths.contiguous().numpy()
    elif isinstance(seqlengths, np.ndarray):
        if seqlengths.dtype != np.int32 or seqlengths.ndim != 1 or not seqlengths.flags["C_CONTIGUOUS"]:
            raise TypeError("seqlengths: expected a C-contiguous 1-d int32 array on the host")
        host = seqlengths
    else:
        raise TypeError("seqlengths: expected a numpy array or CPU tensor (int32)")
    dev = torch.from_numpy(host).to(device, non_blocking=False)
    return host, dev


@_array_args("inputArr")
def hipFastHadamardTransform2D(inputArr):
    """In-place un-normalised FHT over the last axis of a 2-d array
    (cudaFastHadamardTransform2D, xgpr_cuda_rfgen_cpp_ext.cpp:21-24)."""
    s = _ftype(inputArr, "inputArr")
    p = _dev(inputArr, "inputArr", None, 2)
    return _lib.check(getattr(_LIB, f"xgpr_fht_{s}")(p, inputArr.shape[0], 1, inputArr.shape[1], _stream()))


@_array_args("inputArr")
def hipFastHadamardTransform(inputArr):
    """3-d form (cpuFastHadamardTransform, cpu_rf_gen/xgpr_cpu_rfgen_cpp_ext.cpp:24-30)."""
    s = _ftype(inputArr, "inputArr")
    p = _dev(inputArr, "inputArr", None, 3)
    return _lib.check(getattr(_LIB, f"xgpr_fht_{s}")(p, inputArr.shape[0], inputArr.shape[1],
                                                      inputArr.shape[2], _stream()))


@_array_args("inputArr", "radem")
def hipSRHT(inputArr, radem):
    """cudaSRHT (xgpr_cuda_rfgen_cpp_ext.cpp:25-30)."""
    s = _ftype(inputArr, "inputArr")
    p = _dev(inputArr, "inputArr", None, 2)
    r = _dev(radem, "radem", torch.int8, 1)
    return _lib.check(getattr(_LIB, f"xgpr_srht_{s}")(p, r, inputArr.shape[0], inputArr.shape[1],
                                                       radem.shape[0], _stream()))


def _radem3(radem):
    r = _dev(radem, "radem", torch.int8, 3)
    if radem.shape[0] != 3 or radem.shape[1] != 1:
        raise TypeError("radem: expected shape (3, 1, R)")
    return r


@_array_args("inputArr", "radem", "sampler", "outputArr", "yArr", "ztyOut", "workspace")
def hipSRHTSample(inputArr, radem, sampler, outputArr, ncols=None, yArr=None, ztyOut=None, workspace=None):
    """``outputArr[:, :ncols] = cudaSRHT(pad(inputArr))[:, sampler[:ncols]]`` without touching inputArr
    (srht_compressor.py:87-97 in one pass).  outputArr may have more than ncols columns (row pitch).
    With ``yArr`` the same pass also writes ``inputArr.T @ yArr`` into ``ztyOut``."""
    s = _ftype(inputArr, "inputArr")
    x = _dev(inputArr, "inputArr", None, 2)
    r = _dev(radem, "radem", torch.int8, 1)
    sm = _dev(sampler, "sampler", torch.int64, 1)
    o = _dev(outputArr, "outputArr", inputArr.dtype, 2)
    ncols = sampler.shape[0] if ncols is None else int(ncols)
    if outputArr.shape[0] != inputArr.shape[0] or outputArr.shape[1] < ncols or sampler.shape[0] < ncols:
        raise RuntimeError("incorrect array dims passed")
    yp = zp = wp = C.c_void_p(0)
    wn = C.c_size_t(0)
    if yArr is not None:
        yp = _dev(yArr, "yArr", torch.float64, 1)
        zp = _dev(ztyOut, "ztyOut", torch.float64, 1)
        if yArr.shape[0] != inputArr.shape[0] or ztyOut.shape[0] != inputArr.shape[1]:
            raise RuntimeError("incorrect array dims passed")
        if workspace is None:
            workspace = torch.empty(int(_LIB.xgpr_srht_sample_workspace_bytes(inputArr.shape[1])), dtype=torch.uint8,
                                    device=inputArr.device)
        wp, wn = C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel())
    fn = getattr(_LIB, f"xgpr_srht_sample_{s}")
    return _lib.check(fn(x, r, sm, o, yp, zp, inputArr.shape[0], inputArr.shape[1], radem.shape[0], ncols,
                         outputArr.shape[1], wp, wn, _stream()))


@_array_args("cacheArr", "radem", "sampler", "outputArr", "yArr", "ztyOut", "workspace")
def hipSRHTSampleRows(cacheArr, radem, sampler, outputArr, ncols, fitIntercept, scale=0.0, yArr=None, ztyOut=None,
                      workspace=None):
    """SRHTCompressor.transform_x (srht_compressor.py:87-97) + the chunk's z^T y (rand_nys_constructors.py:115) from
    FLOAT32 feature rows (Z = scale * cacheArr, Z[:, 0] = 1 with fitIntercept; scale = 0: the RBF-family constant):
    ``outputArr[:, :ncols] = cudaSRHT(pad(Z))[:, sampler[:ncols]]`` in float64, remaining columns zeroed.  Any padded
    width up to 32768 (rows beyond the LDS capacity go block by block)."""
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    r = _dev(radem, "radem", torch.int8, 1)
    sm = _dev(sampler, "sampler", torch.int64, 1)
    o = _dev(outputArr, "outputArr", torch.float64, 2)
    ncols = int(ncols)
    if outputArr.shape[0] != cacheArr.shape[0] or outputArr.shape[1] < ncols or sampler.shape[0] < ncols:
        raise RuntimeError("incorrect array dims passed")
    yp = zp = wp = C.c_void_p(0)
    wn = C.c_size_t(0)
    if yArr is not None:
        yp = _dev(yArr, "yArr", torch.float64, 1)
        zp = _dev(ztyOut, "ztyOut", torch.float64, 1)
        if yArr.shape[0] != cacheArr.shape[0] or ztyOut.shape[0] != cacheArr.shape[1]:
            raise RuntimeError("incorrect array dims passed")
        if workspace is None:
            workspace = torch.empty(int(_LIB.xgpr_srht_sample_workspace_bytes(cacheArr.shape[1])), dtype=torch.uint8,
                                    device=cacheArr.device)
        wp, wn = C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel())
    return _lib.check(_LIB.xgpr_srht_sample_rows_f32(zc, r, sm, o, yp, zp, cacheArr.shape[0], cacheArr.shape[1],
                                                     radem.shape[0], ncols, outputArr.shape[1], float(scale),
                                                     int(bool(fitIntercept)), wp, wn, _stream()))


def srht_sample_rows_ok(padded_width, ncols, num_rffs):
    """Whether hipSRHTSampleRows covers this shape (see include/xgpr_hip.h)."""
    nb = max(1, padded_width // 8192)
    return padded_width <= 32768 and (nb == 1 or (nb * ncols <= 8192 and num_rffs % 4 == 0))


@_array_args("aMat", "cacheArr", "outArr", "workspace")
def hipSketchGemm(aMat, cacheArr, outArr, nrows, bt, transOut, fitIntercept, scale=0.0, accumulate=False, workspace=None):
    """``outArr (+)= aMat[:, :nrows].T @ Z`` (bt False: aMat [n, lda], outArr [nrows, num_rffs] or transposed) or
    ``aMat[:, :nrows].T @ Z.T`` (bt True: aMat [num_rffs, lda], outArr [nrows, n] or transposed) on the float64 matrix
    cores, Z = scale * cacheArr float32 rows with Z[:, 0] = 1 when fitIntercept -- the dense products of
    rand_nys_constructors.py:34, :54, :119 without a float64 copy of Z.  aMat's row pitch must be a multiple of 64
    with zeros beyond column nrows."""
    ap = _dev(aMat, "aMat", torch.float64, 2)
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    op = _dev(outArr, "outArr", torch.float64, 2)
    n, m = cacheArr.shape
    nrows = int(nrows)
    jdim, kdim = (n, m) if bt else (m, n)
    if aMat.shape[0] != kdim or aMat.shape[1] < nrows:
        raise RuntimeError("incorrect array dims passed")
    want = (jdim, nrows) if transOut else (nrows, jdim)
    if outArr.shape[0] != want[0] or outArr.shape[1] < want[1]:
        raise RuntimeError("incorrect array dims passed")
    need = int(_LIB.xgpr_sketch_gemm_workspace_bytes(nrows, jdim, kdim, outArr.shape[1], int(bool(transOut))))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=cacheArr.device)
    return _lib.check(_LIB.xgpr_sketch_gemm_f64(ap, aMat.shape[1], zc, n, m, op, outArr.shape[1], nrows, int(bool(bt)),
                                                int(bool(transOut)), float(scale), int(bool(fitIntercept)),
                                                int(bool(accumulate)), C.c_void_p(workspace.data_ptr()),
                                                C.c_size_t(workspace.numel()), _stream()))


def gram_ok(num_rffs, msub):
    """Shapes hipZtZGram covers: whole 128 x 128 tiles of the leading msub features."""
    return msub % 128 == 0 and 0 < msub <= num_rffs and num_rffs % 4 == 0


def hipZtZGram(cacheArr, outArr, fitIntercept, scale=0.0, accumulate=False, workspace=None):
    """``outArr[msub, msub] (+)= Z[:, :msub].T @ Z[:, :msub]`` with msub = outArr.shape[0] on the float64 matrix cores,
    Z = scale * cacheArr float32 rows with Z[:, 0] = 1 when fitIntercept (exact_nmll_calcs.py:42-78, :116-139;
    lb_optimizer.py:68-117) -- both operands from the float32 rows, no float64 copy of Z.  Returns the workspace used
    (pass it back in to avoid reallocation)."""
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    op = _dev(outArr, "outArr", torch.float64, 2)
    n, m = cacheArr.shape
    msub = outArr.shape[0]
    if outArr.shape[1] < msub or not gram_ok(m, msub):
        raise RuntimeError("incorrect array dims passed")
    need = int(_LIB.xgpr_ztz_gram_workspace_bytes(msub, n))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=cacheArr.device)
    _lib.check(_LIB.xgpr_ztz_gram_f64(zc, n, m, op, outArr.shape[1], msub, float(scale), int(bool(fitIntercept)),
                                      int(bool(accumulate)), C.c_void_p(workspace.data_ptr()),
                                      C.c_size_t(workspace.numel()), _stream()))
    return workspace


def cross_gram_ok(num_rffs):
    """Shapes hipCrossGram covers: whole 128 x 128 tiles (the rule of ``gram_ok`` with msub = num_rffs)."""
    return gram_ok(num_rffs, num_rffs)


def hipCrossGram(aRows, bRows, outArr, accumulate=False, workspace=None):
    """``outArr[M, M] (+)= aRows.T @ bRows + bRows.T @ aRows`` on the float64 matrix cores from two float32 row arrays
    [n, M] of complete rows (nmll_gradient_tools.py:70 and :88: ``inner_deriv`` after its symmetrisation).  ``outArr``
    is float64 with unit column stride: a contiguous [M, ldc >= M] array or an [M, M] view of one.  Symmetric bit
    for bit, deterministic.  Returns the workspace used (pass it back in to avoid reallocation)."""
    a = _dev(aRows, "aRows", torch.float32, 2)
    b = _dev(bRows, "bRows", torch.float32, 2)
    if not isinstance(outArr, torch.Tensor) or not outArr.is_cuda or outArr.dtype != torch.float64 or outArr.dim() != 2:
        raise TypeError("outArr: expected a 2-d float64 device tensor")
    n, m = aRows.shape
    if tuple(bRows.shape) != (n, m):
        raise TypeError("aRows / bRows: expected the same shape")
    if outArr.stride(1) != 1 or outArr.shape[0] != m or outArr.shape[1] < m or outArr.stride(0) < outArr.shape[1]:
        raise TypeError("outArr: expected [M, >= M] with unit column stride")
    if not cross_gram_ok(m):
        raise RuntimeError("incorrect array dims passed")
    need = int(_LIB.xgpr_cross_gram_workspace_bytes(m, n))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=aRows.device)
    _lib.check(_LIB.xgpr_cross_gram_f64(a, b, n, m, C.c_void_p(outArr.data_ptr()), outArr.stride(0), int(bool(accumulate)),
                                        C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))
    return workspace


def sketch_gemm_workspace_bytes(nrows, jdim, kdim, ldc, trans_out):
    return int(_LIB.xgpr_sketch_gemm_workspace_bytes(nrows, jdim, kdim, ldc, int(bool(trans_out))))


def srht_sample_workspace_bytes(m):
    return int(_LIB.xgpr_srht_sample_workspace_bytes(m))


def srht_sample_ok(padded_width, dtype):
    """Whether hipSRHTSample covers this padded width (the row must fit in LDS)."""
    return padded_width * (8 if dtype == torch.float64 else 4) <= 128 * 1024


@_array_args("inputArr", "outputArr", "radem", "chiArr")
def hipRBFFeatureGen(inputArr, outputArr, radem, chiArr, fitIntercept):
    """cudaRBFFeatureGen (xgpr_cuda_rfgen_cpp_ext.cpp:32-40).  The output is overwritten
    (as by the reference's CUDA kernel, rbf_ops.cu:121-127)."""
    s = _ftype(inputArr, "inputArr")
    x = _dev(inputArr, "inputArr", None, 2)
    o = _dev(outputArr, "outputArr", torch.float64, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", inputArr.dtype, 1)
    ws, wp, wn = _sorf_ws(radem, inputArr.shape[1], inputArr)
    return _lib.check(getattr(_LIB, f"xgpr_rbf_feature_gen_{s}")(
        x, o, r, c, inputArr.shape[0], inputArr.shape[1], outputArr.shape[0], outputArr.shape[1],
        chiArr.shape[0], radem.shape[2], int(bool(fitIntercept)), wp, wn, _stream()))


@_array_args("inputArr", "outputArr", "gradArr", "radem", "chiArr")
def hipRBFGrad(inputArr, outputArr, gradArr, radem, chiArr, sigma, fitIntercept):
    """cudaRBFGrad (xgpr_cuda_rfgen_cpp_ext.cpp:41-49)."""
    s = _ftype(inputArr, "inputArr")
    x = _dev(inputArr, "inputArr", None, 2)
    o = _dev(outputArr, "outputArr", torch.float64, 2)
    g = _dev(gradArr, "gradArr", torch.float64, 3)
    if gradArr.shape[2] != 1:
        raise TypeError("gradArr: expected shape (N, M, 1)")
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", inputArr.dtype, 1)
    ws, wp, wn = _sorf_ws(radem, inputArr.shape[1], inputArr)
    return _lib.check(getattr(_LIB, f"xgpr_rbf_grad_{s}")(
        x, o, g, r, c, inputArr.shape[0], inputArr.shape[1], outputArr.shape[0], outputArr.shape[1],
        gradArr.shape[0], gradArr.shape[1], chiArr.shape[0], radem.shape[2], float(sigma),
        int(bool(fitIntercept)), wp, wn, _stream()))


GRAD_ROWS_MAX_WIDTH = 8192      # padded input width up to which xgpr_rbf_grad_rows_f32 has a plan


def hipRBFGradRows(inputArr, zRows, gRows, radem, chiArr, sigma, fitIntercept):
    """cudaRBFGrad writing float32 rows: ``zRows[N, M]`` and ``gRows[N, M]`` (float32, 8-byte aligned, unit column
    stride, rows of M floats apart; both overwritten) hold what hipRBFGrad writes to ``outputArr`` and
    ``gradArr[:, :, 0]`` -- every entry of those is a float32 value -- with column 0 set to 1 / 0 under fitIntercept:
    complete rows (see include/xgpr_hip.h)."""
    x = _dev(inputArr, "inputArr", torch.float32, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", torch.float32, 1)
    n = inputArr.shape[0]
    for t, nm in ((zRows, "zRows"), (gRows, "gRows")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise TypeError(f"{nm}: expected a 2-d float32 device tensor")
        if t.shape[0] != n:
            raise RuntimeError("no datapoints")
        if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1]):
            raise TypeError(f"{nm}: expected rows of M contiguous floats, M floats apart")
    if tuple(gRows.shape) != tuple(zRows.shape):
        raise RuntimeError("Wrong array sizes.")
    ws, wp, wn = _sorf_ws(radem, inputArr.shape[1], inputArr)
    return _lib.check(_LIB.xgpr_rbf_grad_rows_f32(
        x, C.c_void_p(zRows.data_ptr()), C.c_void_p(gRows.data_ptr()), r, c, n, inputArr.shape[1], zRows.shape[1],
        chiArr.shape[0], radem.shape[2], float(sigma), int(bool(fitIntercept)), wp, wn, _stream()))


@_array_args("inputArr", "outputArr", "precompWeights", "sigmaMap", "sigmaVals", "gradArr")
def hipMiniARDGrad(inputArr, outputArr, precompWeights, sigmaMap, sigmaVals, gradArr, fitIntercept):
    """cudaMiniARDGrad (xgpr_cuda_rfgen_cpp_ext.cpp:50-60)."""
    s = _ftype(inputArr, "inputArr")
    x = _dev(inputArr, "inputArr", None, 2)
    o = _dev(outputArr, "outputArr", torch.float64, 2)
    w = _dev(precompWeights, "precompWeights", inputArr.dtype, 2)
    mp = _dev(sigmaMap, "sigmaMap", torch.int32, 1)
    sv = _dev(sigmaVals, "sigmaVals", torch.float64, 1)
    g = _dev(gradArr, "gradArr", torch.float64, 3)
    fn = getattr(_LIB, f"xgpr_mini_ard_grad_{s}")
    return _lib.check(fn(x, o, w, mp, sv, g, inputArr.shape[0], inputArr.shape[1], outputArr.shape[0],
                         outputArr.shape[1], precompWeights.shape[0], precompWeights.shape[1], sigmaMap.shape[0],
                         sigmaVals.shape[0], gradArr.shape[0], gradArr.shape[1], gradArr.shape[2],
                         int(bool(fitIntercept)), _stream()))


@_array_args("inputArr", "outputArr", "radem", "chiArr")
def hipConv1dFGen(inputArr, outputArr, radem, chiArr, seqlengths, convWidth, scalingType):
    """cudaConv1dFGen (xgpr_cuda_rfgen_cpp_ext.cpp:70-80); results are added into outputArr."""
    s = _ftype(inputArr, "inputArr")
    x = _dev(inputArr, "inputArr", None, 3)
    o = _dev(outputArr, "outputArr", torch.float64, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", inputArr.dtype, 1)
    host, dev = _seqlens(seqlengths, inputArr.device)
    ws, wp, wn = _conv_ws(radem, int(convWidth) * inputArr.shape[2], inputArr)
    return _lib.check(getattr(_LIB, f"xgpr_conv1d_fgen_{s}")(
        x, o, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), inputArr.shape[0],
        inputArr.shape[1], inputArr.shape[2], outputArr.shape[0], outputArr.shape[1], chiArr.shape[0],
        radem.shape[2], host.shape[0], int(convWidth), int(scalingType), wp, wn, _stream()))


@_array_args("inputArr", "rowsArr", "radem", "chiArr")
def hipConvFeatureRows(inputArr, rowsArr, radem, chiArr, seqlengths, convWidth, scalingType, fitIntercept):
    """The float32 feature rows of the sequence kernels (xgpr_conv_feature_rows_f32): rowsArr [N, num_rffs] float32 is
    OVERWRITTEN with what hipConv1dFGen adds into a zeroed float64 array, rounded once to float32, column 0 set to 1
    under ``fitIntercept``.  Argument checks as hipConv1dFGen; float32 input only."""
    x = _dev(inputArr, "inputArr", torch.float32, 3)
    zc = _dev(rowsArr, "rowsArr", torch.float32, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", torch.float32, 1)
    if rowsArr.shape[0] != inputArr.shape[0]:
        raise RuntimeError("no datapoints")
    host, dev = _seqlens(seqlengths, inputArr.device)
    nbytes = _LIB.xgpr_conv_feature_rows_workspace_bytes(radem.shape[2], int(convWidth) * inputArr.shape[2],
                                                         rowsArr.shape[1], inputArr.shape[0])
    ws, wp, wn = _workspace(nbytes, inputArr.device)
    return _lib.check(_LIB.xgpr_conv_feature_rows_f32(
        x, zc, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), inputArr.shape[0], inputArr.shape[1],
        inputArr.shape[2], rowsArr.shape[1], chiArr.shape[0], radem.shape[2], host.shape[0], int(convWidth),
        int(scalingType), int(bool(fitIntercept)), wp, wn, _stream()))


@_array_args("inputArr", "outputArr", "radem", "chiArr", "gradArr")
def hipConvGrad(inputArr, outputArr, radem, chiArr, seqlengths, gradArr, sigma, convWidth, scalingType):
    """cudaConvGrad (xgpr_cuda_rfgen_cpp_ext.cpp:81-92)."""
    s = _ftype(inputArr, "inputArr")
    x = _dev(inputArr, "inputArr", None, 3)
    o = _dev(outputArr, "outputArr", torch.float64, 2)
    g = _dev(gradArr, "gradArr", torch.float64, 3)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", inputArr.dtype, 1)
    host, dev = _seqlens(seqlengths, inputArr.device)
    ws, wp, wn = _conv_ws(radem, int(convWidth) * inputArr.shape[2], inputArr)
    return _lib.check(getattr(_LIB, f"xgpr_conv_grad_{s}")(
        x, o, g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), inputArr.shape[0],
        inputArr.shape[1], inputArr.shape[2], outputArr.shape[0], outputArr.shape[1], gradArr.shape[0],
        gradArr.shape[1], chiArr.shape[0], radem.shape[2], host.shape[0], float(sigma), int(convWidth),
        int(scalingType), wp, wn, _stream()))


@_array_args("inputArr", "zRows", "gRows", "radem", "chiArr")
def hipConvGradRows(inputArr, zRows, gRows, radem, chiArr, seqlengths, sigma, convWidth, scalingType, fitIntercept):
    """cudaConvGrad writing float32 rows (xgpr_conv_grad_rows_f32): ``zRows[N, M]`` and ``gRows[N, M]`` (float32, 8-byte
    aligned, rows of M contiguous floats; both OVERWRITTEN) hold what hipConvGrad adds into zeroed ``outputArr`` and
    ``gradArr[:, :, 0]``, rounded once to float32, with column 0 set to 1 / 0 under fitIntercept: complete rows.  Argument
    checks as hipConvGrad; float32 input only."""
    x = _dev(inputArr, "inputArr", torch.float32, 3)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", torch.float32, 1)
    n = inputArr.shape[0]
    for t, nm in ((zRows, "zRows"), (gRows, "gRows")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise TypeError(f"{nm}: expected a 2-d float32 device tensor")
        if t.shape[0] != n:
            raise RuntimeError("no datapoints")
        if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1]):
            raise TypeError(f"{nm}: expected rows of M contiguous floats, M floats apart")
    if tuple(gRows.shape) != tuple(zRows.shape):
        raise RuntimeError("Wrong array sizes.")
    host, dev = _seqlens(seqlengths, inputArr.device)
    nbytes = _LIB.xgpr_conv_grad_rows_workspace_bytes(radem.shape[2], int(convWidth) * inputArr.shape[2], zRows.shape[1], n)
    ws, wp, wn = _workspace(nbytes, inputArr.device)
    return _lib.check(_LIB.xgpr_conv_grad_rows_f32(
        x, C.c_void_p(zRows.data_ptr()), C.c_void_p(gRows.data_ptr()), r, c, C.c_void_p(host.ctypes.data),
        C.c_void_p(dev.data_ptr()), n, inputArr.shape[1], inputArr.shape[2], zRows.shape[1], chiArr.shape[0],
        radem.shape[2], host.shape[0], float(sigma), int(convWidth), int(scalingType), int(bool(fitIntercept)), wp, wn,
        _stream()))


def conv_token_rows_ok(width, vocab, C):
    """1 where hipConvTokenRows / hipConvTokenGradRows serve a window of ``width`` = conv_width * C elements over a table of
    ``vocab`` rows and ``C`` columns, 0 otherwise (xgpr_conv_token_rows_ok; no device work)."""
    return int(_LIB.xgpr_conv_token_rows_ok(int(width), int(vocab), int(C)))


def _float_rows(t, nm, n):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f"{nm}: expected a 2-d float32 device tensor")
    if t.shape[0] != n:
        raise RuntimeError("no datapoints")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1]):
        raise TypeError(f"{nm}: expected rows of M contiguous floats, M floats apart")
    return C.c_void_p(t.data_ptr())


@_array_args("tokens", "table", "rows_out", "radem", "chi")
def hipConvTokenRows(tokens, table, rows_out, radem, chi, seqlen, conv_width, scaling_type, fit_intercept):
    """hipConvFeatureRows for sequences given as tokens (xgpr_conv_token_rows_f32): ``tokens`` [N, L] uint8 index the rows
    of ``table`` [V, C] float32 (already sigma-scaled), and ``rows_out`` [N, num_rffs] float32 is OVERWRITTEN with exactly the
    rows hipConvFeatureRows writes for the dense array ``table[tokens]``.  Shapes for which ``conv_token_rows_ok`` is 0 raise
    RuntimeError and launch nothing."""
    t = _dev(tokens, "tokens", torch.uint8, 2)
    tab = _dev(table, "table", torch.float32, 2)
    n = tokens.shape[0]
    zc = _float_rows(rows_out, "rows_out", n)
    r = _radem3(radem)
    c = _dev(chi, "chi", torch.float32, 1)
    host, dev = _seqlens(seqlen, tokens.device)
    nbytes = _LIB.xgpr_conv_feature_rows_workspace_bytes(radem.shape[2], int(conv_width) * table.shape[1], rows_out.shape[1], n)
    ws, wp, wn = _workspace(nbytes, tokens.device)
    return _lib.check(_LIB.xgpr_conv_token_rows_f32(
        t, tab, zc, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, tokens.shape[1], table.shape[0],
        table.shape[1], rows_out.shape[1], chi.shape[0], radem.shape[2], host.shape[0], int(conv_width), int(scaling_type),
        int(bool(fit_intercept)), wp, wn, _stream()))


@_array_args("tokens", "table", "zrows", "grows", "radem", "chi")
def hipConvTokenGradRows(tokens, table, zrows, grows, radem, chi, seqlen, sigma, conv_width, scaling_type, fit_intercept):
    """hipConvGradRows for sequences given as tokens (xgpr_conv_token_grad_rows_f32): ``table`` is NOT pre-multiplied by
    sigma; ``zrows`` and ``grows`` are OVERWRITTEN with exactly the rows hipConvGradRows writes for ``table[tokens]``."""
    t = _dev(tokens, "tokens", torch.uint8, 2)
    tab = _dev(table, "table", torch.float32, 2)
    n = tokens.shape[0]
    z = _float_rows(zrows, "zrows", n)
    g = _float_rows(grows, "grows", n)
    if tuple(grows.shape) != tuple(zrows.shape):
        raise RuntimeError("Wrong array sizes.")
    r = _radem3(radem)
    c = _dev(chi, "chi", torch.float32, 1)
    host, dev = _seqlens(seqlen, tokens.device)
    nbytes = _LIB.xgpr_conv_grad_rows_workspace_bytes(radem.shape[2], int(conv_width) * table.shape[1], zrows.shape[1], n)
    ws, wp, wn = _workspace(nbytes, tokens.device)
    return _lib.check(_LIB.xgpr_conv_token_grad_rows_f32(
        t, tab, z, g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, tokens.shape[1], table.shape[0],
        table.shape[1], zrows.shape[1], chi.shape[0], radem.shape[2], host.shape[0], float(sigma), int(conv_width),
        int(scaling_type), int(bool(fit_intercept)), wp, wn, _stream()))


@_array_args("inputArr", "outputArr", "radem", "chiArr")
def hipConv1dMaxpool(inputArr, outputArr, radem, chiArr, seqlengths, convWidth):
    """cudaConv1dMaxpool (xgpr_cuda_rfgen_cpp_ext.cpp:61-69); float32 output."""
    s = _ftype(inputArr, "inputArr")
    x = _dev(inputArr, "inputArr", None, 3)
    o = _dev(outputArr, "outputArr", torch.float32, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", inputArr.dtype, 1)
    host, dev = _seqlens(seqlengths, inputArr.device)
    ws, wp, wn = _conv_ws(radem, int(convWidth) * inputArr.shape[2], inputArr)
    return _lib.check(getattr(_LIB, f"xgpr_conv1d_maxpool_{s}")(
        x, o, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), inputArr.shape[0],
        inputArr.shape[1], inputArr.shape[2], outputArr.shape[0], outputArr.shape[1], chiArr.shape[0],
        radem.shape[2], host.shape[0], int(convWidth), wp, wn, _stream()))


@_array_args("tokens", "table", "outputArr", "radem", "chiArr")
def hipConvTokenMaxpool(tokens, table, outputArr, radem, chiArr, seqlengths, convWidth):
    """hipConv1dMaxpool for sequences given as tokens (xgpr_conv_token_maxpool_f32): ``tokens`` [N, L] uint8 index the rows of
    ``table`` [V, C] float32, and ``outputArr`` [N, num_rffs] float32 becomes max(outputArr, ...) over the k-mers, exactly as
    hipConv1dMaxpool leaves it for the dense array ``table[tokens]`` (the caller zero-fills it).  Shapes for which
    ``conv_token_rows_ok`` is 0 raise RuntimeError and launch nothing."""
    t = _dev(tokens, "tokens", torch.uint8, 2)
    tab = _dev(table, "table", torch.float32, 2)
    o = _dev(outputArr, "outputArr", torch.float32, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", torch.float32, 1)
    host, dev = _seqlens(seqlengths, tokens.device)
    n = tokens.shape[0]
    nbytes = _LIB.xgpr_conv_workspace_bytes(radem.shape[2], int(convWidth) * table.shape[1], 4, n)
    ws, wp, wn = _workspace(nbytes, tokens.device)
    return _lib.check(_LIB.xgpr_conv_token_maxpool_f32(
        t, tab, o, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, tokens.shape[1], table.shape[0],
        table.shape[1], outputArr.shape[0], outputArr.shape[1], chiArr.shape[0], radem.shape[2], host.shape[0], int(convWidth),
        wp, wn, _stream()))


@_array_args("inputArr", "radem", "chiArr", "vec", "outVec", "workspace")
def hipZtZMatvec(inputArr, radem, chiArr, vec, outVec, fitIntercept, workspace=None, masksPacked=False):
    """Fused ``Z.T @ (Z @ vec)`` over one shard of (sigma-scaled, float32) rows: the chunk
    body of the reference's CG matvec (fitting_toolkit/cg_tools.py:189-191) with
    ``kernel.transform_x`` fused in.  ``outVec`` [num_rffs] f64 is overwritten.  ``masksPacked``:
    ``workspace`` still holds the sign masks an earlier call packed from the same ``radem``."""
    x = _dev(inputArr, "inputArr", torch.float32, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", torch.float32, 1)
    v = _dev(vec, "vec", torch.float64, 1)
    o = _dev(outVec, "outVec", torch.float64, 1)
    if vec.shape[0] != outVec.shape[0]:
        raise TypeError("vec / outVec: shapes differ")
    need = _LIB.xgpr_ztz_matvec_workspace_bytes(outVec.shape[0], radem.shape[2])
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=inputArr.device)
    if masksPacked and workspace is not None:
        r = C.c_void_p(0)
    return _lib.check(_LIB.xgpr_ztz_matvec_f32(
        x, r, c, v, o, inputArr.shape[0], inputArr.shape[1], outVec.shape[0], chiArr.shape[0],
        radem.shape[2], int(bool(fitIntercept)), C.c_void_p(workspace.data_ptr()),
        C.c_size_t(workspace.numel()), _stream()))


@_array_args("inputArr", "radem", "chiArr", "yvec", "outVec", "workspace")
def hipZtY(inputArr, radem, chiArr, yvec, outVec, fitIntercept, workspace=None):
    """Fused ``Z.T @ y`` over one shard (scoring_toolkit/exact_nmll_calcs.py:35-37)."""
    x = _dev(inputArr, "inputArr", torch.float32, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", torch.float32, 1)
    y = _dev(yvec, "yvec", torch.float64, 1)
    o = _dev(outVec, "outVec", torch.float64, 1)
    if yvec.shape[0] != inputArr.shape[0]:
        raise TypeError("yvec: one value per datapoint expected")
    need = _LIB.xgpr_ztz_matvec_workspace_bytes(outVec.shape[0], radem.shape[2])
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=inputArr.device)
    return _lib.check(_LIB.xgpr_zty_f32(
        x, r, c, y, o, inputArr.shape[0], inputArr.shape[1], outVec.shape[0], chiArr.shape[0],
        radem.shape[2], int(bool(fitIntercept)), C.c_void_p(workspace.data_ptr()),
        C.c_size_t(workspace.numel()), _stream()))


def _err_ptr(t):
    if t is None:
        return 0
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.numel() < 1 or not (t.is_cuda or t.is_pinned()):
        raise TypeError("err_out: expected a float64 tensor on the device or in pinned host memory")
    return t.data_ptr()


def hipCGStep1(w, p, x, r, r_next, z, scal, lam2, init_norm, stop_tol=0.0, err_out=None):
    """cg_tools.py:256-265 for one right-hand side (see include/xgpr_hip.h).  ``stop_tol`` > 0: the
    convergence test is applied on the device too (iterations queued ahead of the host's check);
    scal then has 8 + max_iterations entries.  ``err_out``: a one-element float64 tensor that also receives
    the error -- on the device, or in pinned host memory (written by the kernel itself, no copy command)."""
    for name, t in (("w", w), ("p", p), ("x", x), ("r", r), ("r_next", r_next), ("z", z)):
        _dev(t, name, torch.float64, 1)
    _dev(scal, "scal", torch.float64, 1)
    return _lib.check(_LIB.xgpr_cg_step1_f64(
        C.c_void_p(w.data_ptr()), C.c_void_p(p.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(r.data_ptr()),
        C.c_void_p(r_next.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(scal.data_ptr()), float(lam2),
        float(init_norm), w.shape[0], float(stop_tol), C.c_void_p(_err_ptr(err_out)), _stream()))


def hipCGStep2(r_next, z_next, p, p_next, scal, stop_tol=0.0):
    """cg_tools.py:271-274 for one right-hand side."""
    for name, t in (("r_next", r_next), ("z_next", z_next), ("p", p), ("p_next", p_next)):
        _dev(t, name, torch.float64, 1)
    return _lib.check(_LIB.xgpr_cg_step2_f64(
        C.c_void_p(r_next.data_ptr()), C.c_void_p(z_next.data_ptr()), C.c_void_p(p.data_ptr()),
        C.c_void_p(p_next.data_ptr()), C.c_void_p(scal.data_ptr()), r_next.shape[0], float(stop_tol), _stream()))


def _blk(t, name, k=None):
    _dev(t, name, torch.float64, 2)
    if k is not None and t.shape[1] != k:
        raise TypeError(f"{name}: expected [M, {k}]")
    return C.c_void_p(t.data_ptr())


def hipSoftmaxResidual(pred, labels):
    """nonlinear_cg_toolkit.py:243-262 on the device in one launch: ``pred`` [n, classes] float64 becomes
    softmax_2.71828(pred) - onehot(labels) in place; returns the loss contribution -sum log(max(p[label], 1e-16))
    as a one-element device tensor."""
    _dev(pred, "pred", torch.float64, 2)
    _dev(labels, "labels", torch.int64, 1)
    n, ncls = pred.shape
    if labels.shape[0] != n:
        raise TypeError("labels: expected [n]")
    parts = torch.empty((n + 255) // 256, dtype=torch.float64, device=pred.device)
    _lib.check(_LIB.xgpr_softmax_residual_f64(C.c_void_p(pred.data_ptr()), C.c_void_p(labels.data_ptr()), n, ncls,
                                              C.c_void_p(parts.data_ptr()), _stream()))
    return parts.sum().reshape(1)


CG_BLOCK_MAX_K = 32


def cg_block_workspace_bytes(m, k):
    return int(_LIB.xgpr_cg_block_workspace_bytes(m, k))


def hipCGStep1Block(w, p, x, r, r_next, z, rz, alpha_out, err_out, init_norm, lam2, workspace):
    """cg_tools.py:256-265 for a block of k <= 32 right-hand sides, all [M, k] row-major (see include/xgpr_hip.h).
    ``rz``, ``alpha_out``, ``init_norm``: float64 [k] on the device; ``err_out``: float64 [k], device or pinned host."""
    m, k = w.shape
    ptrs = [_blk(t, n, k) for t, n in ((w, "w"), (p, "p"), (x, "x"), (r, "r"), (r_next, "r_next"), (z, "z"))]
    for t, n in ((rz, "rz"), (alpha_out, "alpha_out"), (init_norm, "init_norm")):
        _dev(t, n, torch.float64, 1)
    if err_out.dtype != torch.float64 or err_out.numel() != k or not err_out.is_contiguous():
        raise TypeError("err_out: expected float64 [k], contiguous")
    return _lib.check(_LIB.xgpr_cg_step1_block_f64(
        *ptrs, C.c_void_p(rz.data_ptr()), C.c_void_p(alpha_out.data_ptr()), C.c_void_p(err_out.data_ptr()),
        C.c_void_p(init_norm.data_ptr()), float(lam2), m, k, C.c_void_p(workspace.data_ptr()),
        C.c_size_t(workspace.numel()), _stream()))


def hipCGStep2Block(r_next, z_next, p, p_next, rz, beta_out, workspace):
    """cg_tools.py:271-274 for a block of right-hand sides."""
    m, k = r_next.shape
    ptrs = [_blk(t, n, k) for t, n in ((r_next, "r_next"), (z_next, "z_next"), (p, "p"), (p_next, "p_next"))]
    _dev(rz, "rz", torch.float64, 1)
    _dev(beta_out, "beta_out", torch.float64, 1)
    return _lib.check(_LIB.xgpr_cg_step2_block_f64(*ptrs, C.c_void_p(rz.data_ptr()), C.c_void_p(beta_out.data_ptr()),
                                                   m, k, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()),
                                                   _stream()))


PRECOND_UTR_BLOCK_MAX_K = 32


def precond_utr_block_workspace_bytes(m, rank, k):
    return int(_LIB.xgpr_precond_utr_block_workspace_bytes(m, rank, k))


def hipPrecondUtRBlock(u_mat, rmat, tout, workspace=None):
    """``tout[rank, k] = u_mat.T @ rmat`` for a block of k <= 32 right-hand sides (the first product of
    rand_nys_preconditioners.py:66-72; the library's skinny GEMM takes 15x as long at rank 512, k = 26)."""
    _dev(u_mat, "u_mat", torch.float64, 2)
    _dev(rmat, "rmat", torch.float64, 2)
    _dev(tout, "tout", torch.float64, 2)
    m, rank = u_mat.shape
    k = rmat.shape[1]
    if rmat.shape[0] != m or tuple(tout.shape) != (rank, k):
        raise TypeError("hipPrecondUtRBlock: expected rmat [M, k] and tout [rank, k]")
    if workspace is None:
        workspace = torch.empty(precond_utr_block_workspace_bytes(m, rank, k), dtype=torch.uint8, device=u_mat.device)
    return _lib.check(_LIB.xgpr_precond_utr_block_f64(
        C.c_void_p(u_mat.data_ptr()), C.c_void_p(rmat.data_ptr()), C.c_void_p(tout.data_ptr()), m, rank, k,
        C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def precond_apply_block_workspace_bytes(m, rank, k):
    return int(_LIB.xgpr_precond_apply_block_workspace_bytes(m, rank, k))


def hipPrecondApplyBlock(u_mat, inv_eig, prefactor, rmat, zmat, workspace=None):
    """RandNysPreconditioner.batch_matvec for a block of k <= 32 right-hand sides (rand_nys_preconditioners.py:66-72):
    ``zmat <- rmat + U ((inv_eig * prefactor - 1) .* (U^T rmat))``, both products on the float64 matrix cores."""
    _dev(u_mat, "u_mat", torch.float64, 2)
    _dev(inv_eig, "inv_eig", torch.float64, 1)
    _dev(rmat, "rmat", torch.float64, 2)
    _dev(zmat, "zmat", torch.float64, 2)
    m, rank = u_mat.shape
    k = rmat.shape[1]
    if rmat.shape[0] != m or tuple(zmat.shape) != (m, k) or inv_eig.shape[0] != rank or zmat.data_ptr() == rmat.data_ptr():
        raise TypeError("hipPrecondApplyBlock: expected rmat, zmat [M, k] (distinct) and inv_eig [rank]")
    if workspace is None:
        workspace = torch.empty(precond_apply_block_workspace_bytes(m, rank, k), dtype=torch.uint8, device=u_mat.device)
    return _lib.check(_LIB.xgpr_precond_apply_block_f64(
        C.c_void_p(u_mat.data_ptr()), C.c_void_p(inv_eig.data_ptr()), float(prefactor), C.c_void_p(rmat.data_ptr()),
        C.c_void_p(zmat.data_ptr()), m, rank, k, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def hipPrecondApply(u_mat, inv_eig, prefactor, rvec, zvec, workspace=None):
    """RandNysPreconditioner.batch_matvec for one right-hand side
    (preconditioners/rand_nys_preconditioners.py:66-72): zvec <- P^-1 rvec."""
    _dev(u_mat, "u_mat", torch.float64, 2)
    _dev(inv_eig, "inv_eig", torch.float64, 1)
    _dev(rvec, "rvec", torch.float64, 1)
    _dev(zvec, "zvec", torch.float64, 1)
    if u_mat.shape[0] != rvec.shape[0] or u_mat.shape[1] != inv_eig.shape[0] or zvec.shape[0] != rvec.shape[0]:
        raise TypeError("hipPrecondApply: shapes do not match")
    need = _LIB.xgpr_precond_apply_workspace_bytes(u_mat.shape[1])
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=u_mat.device)
    return _lib.check(_LIB.xgpr_precond_apply_f64(
        C.c_void_p(u_mat.data_ptr()), C.c_void_p(inv_eig.data_ptr()), float(prefactor),
        C.c_void_p(rvec.data_ptr()), C.c_void_p(zvec.data_ptr()), u_mat.shape[0], u_mat.shape[1],
        C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def precond_workspace_bytes(rank):
    return int(_LIB.xgpr_precond_apply_workspace_bytes(rank))


def hipRBFFeatureCache(inputArr, cacheArr, radem, chiArr):
    """float32 (cos, sin) pairs before scaling, cacheArr [N, num_rffs] float32 (see include/xgpr_hip.h)."""
    x = _dev(inputArr, "inputArr", torch.float32, 2)
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    r = _radem3(radem)
    c = _dev(chiArr, "chiArr", torch.float32, 1)
    if cacheArr.shape[0] != inputArr.shape[0]:
        raise RuntimeError("no datapoints")
    ws, wp, wn = _sorf_ws(radem, inputArr.shape[1], inputArr)
    return _lib.check(_LIB.xgpr_rbf_feature_cache_f32(
        x, zc, r, c, inputArr.shape[0], inputArr.shape[1], cacheArr.shape[1], chiArr.shape[0], radem.shape[2],
        wp, wn, _stream()))


def hipZCacheMatvecScaled(cacheArr, vec, outVec, scale, workspace):
    """``Z.T @ (Z @ vec)`` with Z = scale * cacheArr (any kernel's float32 feature rows)."""
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    v = _dev(vec, "vec", torch.float64, 1)
    o = _dev(outVec, "outVec", torch.float64, 1)
    if vec.shape[0] != cacheArr.shape[1] or outVec.shape[0] != cacheArr.shape[1]:
        raise TypeError("vec / outVec: expected num_rffs entries")
    return _lib.check(_LIB.xgpr_zcache_matvec_scaled_f32(
        zc, v, o, cacheArr.shape[0], cacheArr.shape[1], float(scale),
        C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def hipZCacheMatvec(cacheArr, vec, outVec, fitIntercept, workspace):
    """``Z.T @ (Z @ vec)`` streamed from the resident feature cache (cg_tools.py:189-191)."""
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    v = _dev(vec, "vec", torch.float64, 1)
    o = _dev(outVec, "outVec", torch.float64, 1)
    if vec.shape[0] != cacheArr.shape[1] or outVec.shape[0] != cacheArr.shape[1]:
        raise TypeError("vec / outVec: expected num_rffs entries")
    return _lib.check(_LIB.xgpr_zcache_matvec_f32(
        zc, v, o, cacheArr.shape[0], cacheArr.shape[1], int(bool(fitIntercept)),
        C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


HALF_CACHE_MAX_FREQS = 8192     # the streaming matvec over binary16 rows: one tile of 1024 frequencies per wave (include/xgpr_hip.h)


def half_cache_ok(num_freqs):
    """Whether hipZCacheMatvecHalf serves rows of ``num_freqs`` frequencies."""
    return 1 <= int(num_freqs) <= HALF_CACHE_MAX_FREQS


def hipRowsToHalf(rows_f32, out_f16):
    """out_f16 <- rows_f32 rounded to IEEE binary16 (round to nearest even, subnormals kept); both [n, num_rffs] (or any
    equal shape), contiguous.  Any float32 row writer followed by this is a source of binary16 rows."""
    if not isinstance(rows_f32, torch.Tensor) or not isinstance(out_f16, torch.Tensor):
        raise TypeError("rows_f32 / out_f16: expected device arrays")
    src = _dev(rows_f32, "rows_f32", torch.float32, rows_f32.dim())
    dst = _dev(out_f16, "out_f16", torch.float16, out_f16.dim())
    if tuple(rows_f32.shape) != tuple(out_f16.shape):
        raise TypeError("out_f16: expected the shape of rows_f32")
    return _lib.check(_LIB.xgpr_rows_pack_f16(src, dst, rows_f32.numel(), _stream()))


def hipZCacheMatvecHalfScaled(cache_f16, vec, out, scale, workspace):
    """``Z.T @ (Z @ vec)`` with Z = scale * cache_f16 widened exactly (any kernel's feature rows rounded to binary16)."""
    zc = _dev(cache_f16, "cache_f16", torch.float16, 2)
    v = _dev(vec, "vec", torch.float64, 1)
    o = _dev(out, "out", torch.float64, 1)
    if vec.shape[0] != cache_f16.shape[1] or out.shape[0] != cache_f16.shape[1]:
        raise TypeError("vec / out: expected num_rffs entries")
    return _lib.check(_LIB.xgpr_zcache_matvec_scaled_f16(
        zc, v, o, cache_f16.shape[0], cache_f16.shape[1], float(scale),
        C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def hipZCacheMatvecHalf(cache_f16, vec, out, fitIntercept, workspace):
    """``Z.T @ (Z @ vec)`` streamed from the resident binary16 feature cache: hipZCacheMatvec over rows rounded by
    hipRowsToHalf (the RBF-family scale, Z[:, 0] = 1 under fitIntercept); float64 products and sums, deterministic."""
    zc = _dev(cache_f16, "cache_f16", torch.float16, 2)
    v = _dev(vec, "vec", torch.float64, 1)
    o = _dev(out, "out", torch.float64, 1)
    if vec.shape[0] != cache_f16.shape[1] or out.shape[0] != cache_f16.shape[1]:
        raise TypeError("vec / out: expected num_rffs entries")
    return _lib.check(_LIB.xgpr_zcache_matvec_f16(
        zc, v, o, cache_f16.shape[0], cache_f16.shape[1], int(bool(fitIntercept)),
        C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def hipZCacheZtY(cacheArr, yvec, outVec, fitIntercept, workspace, scale=0.0):
    """``outVec = Z.T @ yvec`` from float32 feature rows (exact_nmll_calcs.py:35-37 without float64 Z): Z = scale *
    cacheArr with Z[:, 0] = 1 under fitIntercept; scale = 0 selects the RBF-family scale, a positive scale is for caches
    that already hold complete feature rows / scale.  ``workspace``: ztz_workspace_bytes of bytes, as hipZCacheMatvec."""
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    y = _dev(yvec, "yvec", torch.float64, 1)
    o = _dev(outVec, "outVec", torch.float64, 1)
    if yvec.shape[0] != cacheArr.shape[0]:
        raise TypeError("yvec: one value per datapoint expected")
    if outVec.shape[0] != cacheArr.shape[1]:
        raise TypeError("outVec: expected num_rffs entries")
    return _lib.check(_LIB.xgpr_zcache_zty_f32(
        zc, y, o, cacheArr.shape[0], cacheArr.shape[1], int(bool(fitIntercept)), float(scale),
        C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def hipZCacheBlockMatvec(cacheArr, vecs, outVecs, fitIntercept, workspace, scale=0.0, accumulate=False):
    """``outVecs (+)= Z.T @ (Z @ vecs)`` for vecs [num_rffs, k <= 32] on the float64 matrix cores, Z streamed
    from the resident feature cache (cg_tools.py:41-44 with a block of right-hand sides).  scale = 0 selects
    the RBF-family scale; a positive scale is for caches that already hold complete feature rows / scale."""
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    v = _dev(vecs, "vecs", torch.float64, 2)
    o = _dev(outVecs, "outVecs", torch.float64, 2)
    if vecs.shape[0] != cacheArr.shape[1] or tuple(outVecs.shape) != tuple(vecs.shape):
        raise TypeError("vecs / outVecs: expected [num_rffs, k]")
    return _lib.check(_LIB.xgpr_zcache_block_matvec_f32(
        zc, v, o, cacheArr.shape[0], cacheArr.shape[1], vecs.shape[1], int(bool(fitIntercept)), float(scale),
        int(bool(accumulate)), C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def hipZCacheBlockProject(cacheArr, vecs, outArr, fitIntercept, scale=0.0, workspace=None):
    """``outArr[n, k] = Z @ vecs`` (the classifier's ``xd @ wvec``, nonlinear_cg_toolkit.py:251) on the
    float64 matrix cores over the float32 feature rows.  ``workspace`` (zcache_block_project_workspace_bytes; allocated
    here when a short launch would use one and none is passed) lets launches of fewer than 65536 rows split the
    contraction over the features across workgroups."""
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    v = _dev(vecs, "vecs", torch.float64, 2)
    o = _dev(outArr, "outArr", torch.float64, 2)
    if vecs.shape[0] != cacheArr.shape[1] or tuple(outArr.shape) != (cacheArr.shape[0], vecs.shape[1]):
        raise TypeError("vecs: expected [num_rffs, k]; outArr: expected [n, k]")
    if workspace is None:
        need = zcache_block_project_workspace_bytes(cacheArr.shape[0], cacheArr.shape[1], vecs.shape[1])
        if need:
            workspace = torch.empty(need, dtype=torch.uint8, device=cacheArr.device)
    wp, wn = (C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel())) if workspace is not None else (None, C.c_size_t(0))
    return _lib.check(_LIB.xgpr_zcache_block_project_f32(
        zc, v, o, cacheArr.shape[0], cacheArr.shape[1], vecs.shape[1], int(bool(fitIntercept)), float(scale),
        wp, wn, _stream()))


def hipZCacheBlockBackproject(cacheArr, resid, outVecs, fitIntercept, workspace, scale=0.0, accumulate=False):
    """``outVecs[num_rffs, k] (+)= Z.T @ resid`` (the classifier's gradient sums,
    nonlinear_cg_toolkit.py:264-269)."""
    zc = _dev(cacheArr, "cacheArr", torch.float32, 2)
    r = _dev(resid, "resid", torch.float64, 2)
    o = _dev(outVecs, "outVecs", torch.float64, 2)
    if resid.shape[0] != cacheArr.shape[0] or tuple(outVecs.shape) != (cacheArr.shape[1], resid.shape[1]):
        raise TypeError("resid: expected [n, k]; outVecs: expected [num_rffs, k]")
    return _lib.check(_LIB.xgpr_zcache_block_backproject_f32(
        zc, r, o, cacheArr.shape[0], cacheArr.shape[1], resid.shape[1], int(bool(fitIntercept)), float(scale),
        int(bool(accumulate)), C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel()), _stream()))


def zcache_block_project_workspace_bytes(ndatapoints, num_rffs, k):
    return int(_LIB.xgpr_zcache_block_project_workspace_bytes(ndatapoints, num_rffs, k))


def zcache_block_workspace_bytes(ndatapoints, num_rffs, k):
    return int(_LIB.xgpr_zcache_block_workspace_bytes(ndatapoints, num_rffs, k))


def ztz_workspace_bytes(num_rffs, radem_shape2):
    return int(_LIB.xgpr_ztz_matvec_workspace_bytes(num_rffs, radem_shape2))


def ztz_matvec_plan(d, num_freqs):
    """1: single pass on the three-wave kernel, 2: single pass on the two-wave kernel, 3: two feature passes, 0: unsupported
    (xgpr_ztz_matvec_plan; no device work)."""
    return int(_LIB.xgpr_ztz_matvec_plan(int(d), int(num_freqs)))


def _grad_weights(weights, n):
    """(row stride for the C ABI, columns available) of an input-gradient weight argument: 1-d, one vector for all rows (stride
    0), or 2-d [n, stride] with unit column stride."""
    if not isinstance(weights, torch.Tensor) or not weights.is_cuda or weights.dtype != torch.float64:
        raise TypeError("weights: expected a float64 device tensor")
    if weights.dim() == 1:
        if not weights.is_contiguous():
            raise TypeError("weights: expected a C-contiguous array")
        stride, avail = 0, weights.shape[0]
    elif weights.dim() == 2:
        if weights.shape[0] != n:
            raise RuntimeError("Wrong array sizes.")
        if weights.stride(1) != 1 or (n > 1 and weights.stride(0) < weights.shape[1]):
            raise TypeError("weights: expected rows of contiguous float64 values")
        stride, avail = (weights.stride(0) if n > 1 else weights.shape[1]), weights.shape[1]
    else:
        raise TypeError("weights: expected 1 or 2 dims")
    return stride, avail


def rbf_input_grad_ok(d, num_freqs):
    """Whether hipRBFInputGrad's kernel serves an input of ``d`` columns (padded width up to 1024); no device work."""
    return int(_LIB.xgpr_rbf_input_grad_ok(int(d), int(num_freqs)))


def hipRBFInputGrad(x_scaled, weights, out, radem, chi, sigma, fit_intercept, w_cols=None, workspace=None):
    """``out[n, d]`` (float64, overwritten) <- d/dx of ``features(x) @ weights`` for the fixed-vector kernels, through the
    transposed SORF (include/xgpr_hip_input_grad.h).  ``x_scaled`` [n, d] float32 is already multiplied by sigma, as for the
    feature operators.  ``weights`` float64: 1-d, one vector for all rows, or 2-d [n, stride] with unit column stride, one
    vector per row (what lies past ``w_cols`` in a row is never read).  Only the first ``w_cols`` feature columns carry
    weight (even; default: all of them).  Under fit_intercept ``weights[..., 0]`` is ignored (column 0 is the constant 1)."""
    x = _dev(x_scaled, "x_scaled", torch.float32, 2)
    g = _dev(out, "out", torch.float64, 2)
    r = _radem3(radem)
    c = _dev(chi, "chi", torch.float32, 1)
    n, d = x_scaled.shape
    if tuple(out.shape) != (n, d):
        raise RuntimeError("Wrong array sizes.")
    stride, avail = _grad_weights(weights, n)
    w_cols = 2 * chi.shape[0] if w_cols is None else int(w_cols)
    if w_cols > avail:
        raise RuntimeError("Wrong array sizes.")
    if workspace is None:
        ws, wp, wn = _workspace(_LIB.xgpr_rbf_workspace_bytes(radem.shape[2]), x_scaled.device)
    else:
        ws, wp, wn = workspace, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel() * workspace.element_size())
    return _lib.check(_LIB.xgpr_rbf_input_grad_f32(
        x, C.c_void_p(weights.data_ptr()), g, r, c, n, d, stride, w_cols, chi.shape[0], radem.shape[2], float(sigma),
        int(bool(fit_intercept)), wp, wn, _stream()))


def conv_input_grad_ok(width, num_freqs):
    """Whether hipConvInputGrad's kernel serves a window of ``width`` = conv_width * C elements (padded width up to 1024)."""
    return int(_LIB.xgpr_conv_input_grad_ok(int(width), int(num_freqs)))


def conv_token_input_grad_ok(width, vocab, C):
    """Whether hipConvTokenInputGrad serves the window and holds a table of ``vocab`` rows and ``C`` columns in LDS."""
    return int(_LIB.xgpr_conv_token_input_grad_ok(int(width), int(vocab), int(C)))


def _seq_grad_tail(weights, n, chi, radem, w_cols, workspace, device):
    stride, avail = _grad_weights(weights, n)
    w_cols = 2 * chi.shape[0] if w_cols is None else int(w_cols)
    if w_cols > avail:
        raise RuntimeError("Wrong array sizes.")
    if workspace is None:
        ws, wp, wn = _workspace(_LIB.xgpr_rbf_workspace_bytes(radem.shape[2]), device)
    else:
        ws, wp, wn = workspace, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel() * workspace.element_size())
    return stride, w_cols, ws, wp, wn


def hipConvInputGrad(x_scaled, weights, out, radem, chi, seqlen, sigma, conv_width, scaling_type, fit_intercept, w_cols=None,
                     workspace=None):
    """``out[n, L, C]`` (float64, OVERWRITTEN; exactly 0.0 at positions past a sequence's length) <- d/dx of
    ``features(x) @ weights`` for the sequence and graph kernels (include/xgpr_hip_seq_input_grad.h): the transposed SORF of
    every k-mer window, overlap-added per position.  ``x_scaled`` [n, L, C] float32 is already multiplied by sigma; ``weights``,
    ``w_cols`` and ``fit_intercept`` as for hipRBFInputGrad; ``seqlen`` int32 on the host."""
    x = _dev(x_scaled, "x_scaled", torch.float32, 3)
    g = _dev(out, "out", torch.float64, 3)
    r = _radem3(radem)
    c = _dev(chi, "chi", torch.float32, 1)
    n, L, ch = x_scaled.shape
    if tuple(out.shape) != (n, L, ch):
        raise RuntimeError("Wrong array sizes.")
    host, dev = _seqlens(seqlen, x_scaled.device)
    if host.shape[0] != n:
        raise RuntimeError("wrong array sizes")
    stride, w_cols, ws, wp, wn = _seq_grad_tail(weights, n, chi, radem, w_cols, workspace, x_scaled.device)
    return _lib.check(_LIB.xgpr_conv_input_grad_f32(
        x, C.c_void_p(weights.data_ptr()), g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L, ch, stride,
        w_cols, chi.shape[0], radem.shape[2], float(sigma), int(conv_width), int(scaling_type), int(bool(fit_intercept)), wp, wn,
        _stream()))


def hipConvTokenInputGrad(tokens, table, weights, out, radem, chi, seqlen, sigma, conv_width, scaling_type, fit_intercept,
                          w_cols=None, workspace=None):
    """hipConvInputGrad for sequences given as tokens: ``tokens`` [n, L] uint8 index the rows of ``table`` [V, C] float32
    (already sigma-scaled); ``out`` [n, L, C] receives exactly what hipConvInputGrad writes for ``table[tokens]``.  Shapes for
    which ``conv_token_input_grad_ok`` is 0 raise RuntimeError and launch nothing."""
    t = _dev(tokens, "tokens", torch.uint8, 2)
    tab = _dev(table, "table", torch.float32, 2)
    g = _dev(out, "out", torch.float64, 3)
    r = _radem3(radem)
    c = _dev(chi, "chi", torch.float32, 1)
    n, L = tokens.shape
    if tuple(out.shape) != (n, L, table.shape[1]):
        raise RuntimeError("Wrong array sizes.")
    host, dev = _seqlens(seqlen, tokens.device)
    if host.shape[0] != n:
        raise RuntimeError("wrong array sizes")
    stride, w_cols, ws, wp, wn = _seq_grad_tail(weights, n, chi, radem, w_cols, workspace, tokens.device)
    return _lib.check(_LIB.xgpr_conv_token_input_grad_f32(
        t, tab, C.c_void_p(weights.data_ptr()), g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L,
        table.shape[0], table.shape[1], stride, w_cols, chi.shape[0], radem.shape[2], float(sigma), int(conv_width),
        int(scaling_type), int(bool(fit_intercept)), wp, wn, _stream()))


def _scan_operands(tokens, table, weights, radem, chi, seqlen, workspace):
    ops = (_dev(tokens, "tokens", torch.uint8, 2), _dev(table, "table", torch.float32, 2), _dev(weights, "weights", torch.float64, 1),
           _radem3(radem), _dev(chi, "chi", torch.float32, 1))
    if weights.shape[0] != 2 * chi.shape[0]:
        raise RuntimeError("Wrong array sizes.")
    host, dev = _seqlens(seqlen, tokens.device)
    if host.shape[0] != tokens.shape[0]:
        raise RuntimeError("wrong array sizes")
    if workspace is None:
        ws, wp, wn = _workspace(_LIB.xgpr_rbf_workspace_bytes(radem.shape[2]), tokens.device)
    else:
        ws, wp, wn = workspace, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel() * workspace.element_size())
    return ops, host, dev, ws, wp, wn


def conv_token_subst_scan_ok(width, vocab, C, num_freqs):
    """Whether hipConvTokenSubstScan's kernel serves a window of ``width`` = conv_width * C elements over a table of ``vocab``
    rows and ``C`` columns (padded width up to 1024, a table the LDS image holds); no device work."""
    return int(_LIB.xgpr_conv_token_subst_scan_ok(int(width), int(vocab), int(C), int(num_freqs)))


def hipConvTokenSubstScan(tokens, table, weights, out, radem, chi, seqlen, conv_width, scaling_type, fit_intercept, workspace=None):
    """``out[n, L, V]`` (float64, OVERWRITTEN) <- ``features(sequence with token l replaced by v) @ weights`` minus
    ``features(sequence) @ weights`` for every position l and token v of the sequence and graph kernels
    (include/xgpr_hip_subst_scan.h): exactly +0.0 at a sequence's own token and past its length.  ``tokens`` [n, L] uint8 index
    the rows of ``table`` [V, C] float32 (already sigma-scaled); ``weights`` float64 [2 * num_freqs], one vector for all
    sequences (``weights[0]`` is ignored under fit_intercept); ``seqlen`` int32 on the host.  Shapes for which
    ``conv_token_subst_scan_ok`` is 0 raise RuntimeError and launch nothing."""
    (t, tab, w, r, c), host, dev, ws, wp, wn = _scan_operands(tokens, table, weights, radem, chi, seqlen, workspace)
    g = _dev(out, "out", torch.float64, 3)
    n, L = tokens.shape
    if tuple(out.shape) != (n, L, table.shape[0]):
        raise RuntimeError("Wrong array sizes.")
    return _lib.check(_LIB.xgpr_conv_token_subst_scan_f32(
        t, tab, w, g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L, table.shape[0], table.shape[1],
        chi.shape[0], radem.shape[2], int(conv_width), int(scaling_type), int(bool(fit_intercept)), wp, wn, _stream()))


def conv_token_pair_scan_ok(width, vocab, C, num_freqs):
    """Whether hipConvTokenPairScan's kernels serve a window of ``width`` = conv_width * C elements over a table of ``vocab`` rows
    and ``C`` columns (where ``conv_token_subst_scan_ok`` is 1); no device work."""
    return int(_LIB.xgpr_conv_token_pair_scan_ok(int(width), int(vocab), int(C), int(num_freqs)))


def hipConvTokenPairScan(tokens, table, weights, out, radem, chi, seqlen, conv_width, scaling_type, fit_intercept, workspace=None):
    """``out[n, L, conv_width - 1, V, V]`` (float64, OVERWRITTEN) <- the non-additive part of every pair of substitutions closer
    than conv_width: ``out[i, l1, d - 1, v1, v2]`` is ``features(sequence with token l1 replaced by v1 and token l1 + d by v2) @
    weights`` minus ``features(sequence) @ weights`` minus the two single effects of hipConvTokenSubstScan
    (include/xgpr_hip_pair_scan.h): exactly +0.0 where either token is the sequence's own and where either position is past its
    length.  Operands as for hipConvTokenSubstScan.  With conv_width 1 ``out`` has no elements and nothing is launched.  Shapes
    for which ``conv_token_pair_scan_ok`` is 0, and batches with n * L * (conv_width - 1) * V >= 2^24, raise RuntimeError and launch
    nothing."""
    (t, tab, w, r, c), host, dev, ws, wp, wn = _scan_operands(tokens, table, weights, radem, chi, seqlen, workspace)
    g = _dev(out, "out", torch.float64, 5)
    n, L = tokens.shape
    V = table.shape[0]
    if tuple(out.shape) != (n, L, int(conv_width) - 1, V, V):
        raise RuntimeError("Wrong array sizes.")
    return _lib.check(_LIB.xgpr_conv_token_pair_scan_f32(
        t, tab, w, g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L, V, table.shape[1],
        chi.shape[0], radem.shape[2], int(conv_width), int(scaling_type), int(bool(fit_intercept)), wp, wn, _stream()))


def conv_token_site_scan_ok(width, vocab, C, num_freqs, max_cover):
    """Whether hipConvTokenSiteScan's kernels serve a window of ``width`` = conv_width * C elements over a table of ``vocab`` rows
    and ``C`` columns (where ``conv_token_subst_scan_ok`` is 1) with at most ``max_cover`` (1 .. 4) sites inside one window; no
    device work."""
    return int(_LIB.xgpr_conv_token_site_scan_ok(int(width), int(vocab), int(C), int(num_freqs), int(max_cover)))


def _site_list(sites):
    s = np.asarray(sites)
    if s.ndim != 1 or s.dtype.kind not in "iu":
        raise TypeError("sites: expected a 1-d sequence of integer positions")
    return np.ascontiguousarray(s.astype(np.int32))


def conv_token_site_scan_layout(sites, L, conv_width, vocab):
    """The runs of a site list on the host (include/xgpr_hip/site_scan.h) -> (runs, T): ``runs`` a list of dicts ``first_window``,
    ``last_window``, ``first_site`` (an index into ``sites``), ``sites`` (their number g) and ``offset`` into a row of
    hipConvTokenSiteScan's output, in ascending window order; ``T`` the length of such a row, the sum of vocab^g.  A site list the
    library refuses (empty, more than 16 sites, not strictly ascending, a site outside 0 .. L - 1) raises RuntimeError."""
    s = _site_list(sites)
    K = s.shape[0]
    cap = max(2 * K - 1, 1)
    i32 = [np.zeros(cap, dtype=np.int32) for _ in range(4)]
    off = np.zeros(cap, dtype=np.int64)
    nr = int(_LIB.xgpr_conv_token_site_scan_layout(C.c_void_p(s.ctypes.data), K, int(L), int(conv_width), int(vocab),
                                                   *[C.c_void_p(a.ctypes.data) for a in i32], C.c_void_p(off.ctypes.data), cap))
    if nr < 0:
        _lib.check(nr)
    runs = [dict(first_window=int(i32[0][q]), last_window=int(i32[1][q]), first_site=int(i32[2][q]), sites=int(i32[3][q]),
                 offset=int(off[q])) for q in range(nr)]
    return runs, (runs[-1]["offset"] + int(vocab) ** runs[-1]["sites"] if runs else 0)


def hipConvTokenSiteScan(tokens, table, weights, out, radem, chi, seqlen, sites, conv_width, scaling_type, fit_intercept, workspace=None):
    """``out[n, T]`` (float64, OVERWRITTEN) <- the run tables of the combinatorial site scan (include/xgpr_hip/site_scan.h): for
    the runs of ``conv_token_site_scan_layout(sites, L, conv_width, V)``, ``out[i, offset + idx]`` is the summed change of the
    run's windows under the assignment ``idx`` of the run's sites, and the sum of one entry per run is ``features(sequence with
    all K sites assigned) @ weights`` minus ``features(sequence) @ weights`` exactly.  Exactly +0.0 at the sequence's own tokens
    and in a run that has no window inside the sequence.  ``sites``: strictly ascending positions on the host, shared by all
    sequences and inside every one of them; the other operands as for hipConvTokenSubstScan.  Shapes for which
    ``conv_token_site_scan_ok`` is 0 -- more than 4 sites inside one window among them -- and batches of 2^24 grid rows or more
    raise RuntimeError and launch nothing."""
    ops = (_dev(tokens, "tokens", torch.uint8, 2), _dev(table, "table", torch.float32, 2), _dev(weights, "weights", torch.float64, 1),
           _radem3(radem), _dev(chi, "chi", torch.float32, 1))
    g = _dev(out, "out", torch.float64, 2)
    if weights.shape[0] != 2 * chi.shape[0]:
        raise RuntimeError("Wrong array sizes.")
    s = _site_list(sites)
    n, L = tokens.shape
    V = table.shape[0]
    # (a site list or a shape the layout refuses is left to the launcher, which reports it in its documented order)
    nr = int(_LIB.xgpr_conv_token_site_scan_layout(C.c_void_p(s.ctypes.data), s.shape[0], L, int(conv_width), V, None, None, None, None,
                                                   None, 0))
    if nr >= 0 and tuple(out.shape) != (n, conv_token_site_scan_layout(s, L, conv_width, V)[1]):
        raise RuntimeError("Wrong array sizes.")
    host, dev = _seqlens(seqlen, tokens.device)
    if host.shape[0] != n:
        raise RuntimeError("wrong array sizes")
    if workspace is None:
        ws, wp, wn = _workspace(_LIB.xgpr_conv_token_site_scan_workspace_bytes(radem.shape[2], n, s.shape[0]), tokens.device)
    else:
        ws, wp, wn = workspace, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel() * workspace.element_size())
    return _lib.check(_LIB.xgpr_conv_token_site_scan_f32(
        *ops[:3], g, *ops[3:], C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), C.c_void_p(s.ctypes.data), s.shape[0], n, L, V,
        table.shape[1], chi.shape[0], radem.shape[2], int(conv_width), int(scaling_type), int(bool(fit_intercept)), wp, wn, _stream()))


def _var_scan_nvar(vm):
    """``vm`` of hipConvTokenSubstVarScan and hipConvTokenIndelVarScan, checked: -> nvar."""
    if vm.dim() != 2 or vm.dtype != torch.float64 or not vm.is_cuda or vm.shape[0] != vm.shape[1] or vm.stride(1) != 1:
        raise RuntimeError("vm must be a float64 device matrix [nvar, nvar] with contiguous rows.")
    return vm.shape[0]


def _var_scan_workspace(tokens, radem, seqlen, nvar, mutants, slab_rows, workspace, workspace_bytes):
    """The host lengths, the slab and the workspace of a variance scan whose largest row set has ``mutants`` rows
    (``workspace_bytes``: the operator's own function): -> (host, dev, slab_rows, ws, wp, wn)."""
    host, dev = _seqlens(seqlen, tokens.device)
    if host.shape[0] != tokens.shape[0]:
        raise RuntimeError("wrong array sizes")
    if workspace is None:
        if slab_rows == 0 and nvar >= 2 and nvar % 2 == 0:
            # (a call with fewer mutant rows than the default slab holds allocates no more than its rows: the slab size does not enter the result)
            masks = int(_LIB.xgpr_rbf_workspace_bytes(radem.shape[2]))
            default = (workspace_bytes(radem.shape[2], nvar, 0) - masks) // (8 * nvar)
            rows = max(16, -(-mutants // 16) * 16)
            slab_rows = rows if rows < default else 0
        ws, wp, wn = _workspace(workspace_bytes(radem.shape[2], nvar, slab_rows), tokens.device)
    else:
        ws, wp, wn = workspace, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel() * workspace.element_size())
    return host, dev, slab_rows, ws, wp, wn


def conv_token_subst_var_scan_ok(width, vocab, C, num_freqs, nvar):
    """Whether hipConvTokenSubstVarScan's kernels serve the shape: where ``conv_token_subst_scan_ok`` is 1 and ``nvar`` is even,
    at least 2 and at most min(2 * num_freqs, 2048); no device work."""
    return int(_LIB.xgpr_conv_token_subst_var_scan_ok(int(width), int(vocab), int(C), int(num_freqs), int(nvar)))


def conv_token_subst_var_scan_workspace_bytes(radem_shape2, nvar, slab_rows=0):
    """The exact workspace of hipConvTokenSubstVarScan in bytes: the packed sign masks and ``slab_rows`` float64 rows of ``nvar``
    columns (0: the library's default)."""
    return int(_LIB.xgpr_conv_token_subst_var_scan_workspace_bytes(int(radem_shape2), int(nvar), int(slab_rows)))


def hipConvTokenSubstVarScan(tokens, table, vm, u, q, out, radem, chi, seqlen, conv_width, scaling_type, fit_intercept, slab_rows=0,
                             workspace=None):
    """``out[n, L, V]`` (float64, OVERWRITTEN) <- ``z'^T vm z'`` over the first ``nvar = vm.shape[0]`` feature columns z' of the
    sequence with token l replaced by v, for every position l and token v of the sequence and graph kernels
    (include/xgpr_hip_subst_var_scan.h): ``q[i]`` bit for bit at a sequence's own token, exactly 0.0 past its length.  ``vm``
    float64 [nvar, nvar] (rows may be strided; nvar even), ``u`` [n, nvar] = the sequences' columns times vm and ``q`` [n] = their
    quadratic forms, both float64 and precomputed by the caller.  ``slab_rows`` mutant rows are held in the workspace at a time
    (0: the default -- the library's, or the call's own n L V rows where those are fewer --; otherwise a multiple of 16; the result
    does not depend on it).  Shapes for which ``conv_token_subst_var_scan_ok`` is 0 raise RuntimeError and launch nothing."""
    t, tab = _dev(tokens, "tokens", torch.uint8, 2), _dev(table, "table", torch.float32, 2)
    r, c = _radem3(radem), _dev(chi, "chi", torch.float32, 1)
    g = _dev(out, "out", torch.float64, 3)
    n, L = tokens.shape
    nvar = _var_scan_nvar(vm)
    uu, qq = _dev(u, "u", torch.float64, 2), _dev(q, "q", torch.float64, 1)
    if tuple(out.shape) != (n, L, table.shape[0]) or tuple(u.shape) != (n, nvar) or q.shape[0] != n:
        raise RuntimeError("Wrong array sizes.")
    host, dev, slab_rows, ws, wp, wn = _var_scan_workspace(tokens, radem, seqlen, nvar, n * L * table.shape[0], slab_rows, workspace,
                                                           conv_token_subst_var_scan_workspace_bytes)
    return _lib.check(_LIB.xgpr_conv_token_subst_var_scan_f32(
        t, tab, C.c_void_p(vm.data_ptr()), vm.stride(0), uu, qq, g, r, c, C.c_void_p(host.ctypes.data),
        C.c_void_p(dev.data_ptr()), n, L, table.shape[0], table.shape[1], chi.shape[0], radem.shape[2], nvar, int(conv_width),
        int(scaling_type), int(bool(fit_intercept)), int(slab_rows), wp, wn, _stream()))


def conv_token_indel_scan_ok(width, vocab, C, num_freqs):
    """Whether the kernels of hipConvTokenWindowScores / hipConvTokenIndelScan serve a window of ``width`` = conv_width * C elements over
    a table of ``vocab`` rows and ``C`` columns (where ``conv_token_subst_scan_ok`` is 1); no device work."""
    return int(_LIB.xgpr_conv_token_indel_scan_ok(int(width), int(vocab), int(C), int(num_freqs)))


def hipConvTokenWindowScores(tokens, table, weights, scores, radem, chi, seqlen, conv_width, fit_intercept, workspace=None):
    """``scores[n, L]`` (float64, OVERWRITTEN) <- the score of every k-mer window of the sequence and graph kernels
    (include/xgpr_hip_indel_scan.h): ``scores[i, j] = sum_f (w[2f] cos p_f + w[2f+1] sin p_f)`` over the projections p of window j,
    exactly +0.0 for j >= nk.  ``sqrt(1 / num_freqs) / {1, sqrt(nk), nk} * scores[i].sum()`` (+ ``weights[0]`` under fit_intercept) is
    ``features(sequence i) @ weights``.  Operands as for hipConvTokenSubstScan."""
    (t, tab, w, r, c), host, dev, ws, wp, wn = _scan_operands(tokens, table, weights, radem, chi, seqlen, workspace)
    g = _dev(scores, "scores", torch.float64, 2)
    if tuple(scores.shape) != tuple(tokens.shape):
        raise RuntimeError("Wrong array sizes.")
    n, L = tokens.shape
    return _lib.check(_LIB.xgpr_conv_token_window_scores_f32(
        t, tab, w, g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L, table.shape[0], table.shape[1],
        chi.shape[0], radem.shape[2], int(conv_width), int(bool(fit_intercept)), wp, wn, _stream()))


def hipConvTokenIndelScan(tokens, table, weights, scores, deletions, insertions, radem, chi, seqlen, conv_width, scaling_type,
                          fit_intercept, workspace=None):
    """``deletions[n, L]`` <- ``features(sequence without token p) @ weights`` minus ``features(sequence) @ weights``, and
    ``insertions[n, L + 1, V]`` <- the same for the sequence with table row v inserted before position g (g = length appends); both
    float64 and OVERWRITTEN, exactly +0.0 past a sequence's length, quiet NaN for the deletions of a sequence of conv_width tokens
    (include/xgpr_hip_indel_scan.h).  ``scores`` [n, L] float64 is what hipConvTokenWindowScores wrote for the same operands.  Either
    output may be None (that half is skipped), not both.  Shapes for which ``conv_token_indel_scan_ok`` is 0 raise RuntimeError and
    launch nothing."""
    (t, tab, w, r, c), host, dev, ws, wp, wn = _scan_operands(tokens, table, weights, radem, chi, seqlen, workspace)
    n, L = tokens.shape
    sc = _dev(scores, "scores", torch.float64, 2)
    d = _dev(deletions, "deletions", torch.float64, 2) if deletions is not None else None
    g = _dev(insertions, "insertions", torch.float64, 3) if insertions is not None else None
    if tuple(scores.shape) != (n, L) or (deletions is not None and tuple(deletions.shape) != (n, L)) \
            or (insertions is not None and tuple(insertions.shape) != (n, L + 1, table.shape[0])):
        raise RuntimeError("Wrong array sizes.")
    return _lib.check(_LIB.xgpr_conv_token_indel_scan_f32(
        t, tab, w, sc, d, g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L, table.shape[0], table.shape[1],
        chi.shape[0], radem.shape[2], int(conv_width), int(scaling_type), int(bool(fit_intercept)), wp, wn, _stream()))


def conv_token_indel_var_scan_ok(width, vocab, C, num_freqs, nvar):
    """Whether hipConvTokenIndelVarScan's kernels serve the shape: where ``conv_token_indel_scan_ok`` is 1 and ``nvar`` is even,
    at least 2 and at most min(2 * num_freqs, 2048); no device work."""
    return int(_LIB.xgpr_conv_token_indel_var_scan_ok(int(width), int(vocab), int(C), int(num_freqs), int(nvar)))


def conv_token_indel_var_scan_workspace_bytes(radem_shape2, nvar, slab_rows=0):
    """The exact workspace of hipConvTokenIndelVarScan in bytes: the packed sign masks and ``slab_rows`` float64 rows of ``nvar``
    columns (0: the library's default)."""
    return int(_LIB.xgpr_conv_token_indel_var_scan_workspace_bytes(int(radem_shape2), int(nvar), int(slab_rows)))


def hipConvTokenIndelVarScan(tokens, table, vm, u_del, q_del, u_ins, q_ins, deletions, insertions, radem, chi, seqlen, conv_width,
                             scaling_type, fit_intercept, slab_rows=0, workspace=None):
    """``deletions[n, L]`` <- ``z'^T vm z'`` over the first ``nvar = vm.shape[0]`` feature columns z' of the sequence without its
    token at p, and ``insertions[n, L + 1, V]`` <- the same for the sequence with table row v inserted before position g (g = length
    appends); both float64 and OVERWRITTEN, exactly +0.0 past a sequence's length, quiet NaN for the deletions of a sequence of
    conv_width tokens (include/xgpr_hip_indel_var_scan.h).  ``vm`` float64 [nvar, nvar] (rows may be strided; nvar even);
    ``u_del``, ``u_ins`` [n, nvar] = 1/2 (vm + vm^T) b and ``q_del``, ``q_ins`` [n] = b^T vm b for the sequences' rescaled columns
    b = rho z + (1 - rho) e0 with each row set's own rho, float64 and precomputed by the caller.  Either group (u, q, output) may be
    None as a whole (that half is skipped), not both.  ``slab_rows`` mutant rows are held in the workspace at a time (0: the default
    -- the library's, or the call's own rows where those are fewer --; otherwise a multiple of 16; the result does not depend on it).
    Shapes for which ``conv_token_indel_var_scan_ok`` is 0 raise RuntimeError and launch nothing."""
    t, tab = _dev(tokens, "tokens", torch.uint8, 2), _dev(table, "table", torch.float32, 2)
    r, c = _radem3(radem), _dev(chi, "chi", torch.float32, 1)
    n, L = tokens.shape
    V = table.shape[0]
    nvar = _var_scan_nvar(vm)
    ptrs = []
    for u, q, out, shape, what in ((u_del, q_del, deletions, (n, L), "deletions"), (u_ins, q_ins, insertions, (n, L + 1, V), "insertions")):
        given = [x is not None for x in (u, q, out)]
        if not any(given):
            ptrs.append((None, None, None))
            continue
        if not all(given):
            raise RuntimeError(f"{what}: u, q and the output are given together or not at all.")
        ptrs.append((_dev(u, "u", torch.float64, 2), _dev(q, "q", torch.float64, 1), _dev(out, what, torch.float64, len(shape))))
        if tuple(out.shape) != shape or tuple(u.shape) != (n, nvar) or q.shape[0] != n:
            raise RuntimeError("Wrong array sizes.")
    host, dev, slab_rows, ws, wp, wn = _var_scan_workspace(tokens, radem, seqlen, nvar, n * (L + 1) * V, slab_rows, workspace,
                                                           conv_token_indel_var_scan_workspace_bytes)
    (ud, qd, od), (ui, qi, oi) = ptrs
    return _lib.check(_LIB.xgpr_conv_token_indel_var_scan_f32(
        t, tab, C.c_void_p(vm.data_ptr()), vm.stride(0), ud, qd, ui, qi, od, oi, r, c, C.c_void_p(host.ctypes.data),
        C.c_void_p(dev.data_ptr()), n, L, V, table.shape[1], chi.shape[0], radem.shape[2], nvar, int(conv_width),
        int(scaling_type), int(bool(fit_intercept)), int(slab_rows), wp, wn, _stream()))


def conv_token_edit_proj_ok(width, vocab, C, num_freqs, nvar, K):
    """Whether the kernels of hipConvTokenSubstProj / hipConvTokenIndelProj serve the shape: where
    ``conv_token_subst_var_scan_ok`` is 1 and 1 <= K <= 2048; no device work."""
    return int(_LIB.xgpr_conv_token_edit_proj_ok(int(width), int(vocab), int(C), int(num_freqs), int(nvar), int(K)))


def conv_token_edit_proj_workspace_bytes(radem_shape2, nvar, slab_rows=0):
    """The exact workspace of hipConvTokenSubstProj / hipConvTokenIndelProj in bytes -- that of the variance scans: the packed sign
    masks and ``slab_rows`` float64 rows of ``nvar`` columns (0: the library's default)."""
    return int(_LIB.xgpr_conv_token_edit_proj_workspace_bytes(int(radem_shape2), int(nvar), int(slab_rows)))


def _proj_matrix(pm):
    """``pm`` of hipConvTokenSubstProj and hipConvTokenIndelProj, checked: -> (nvar, K)."""
    if pm.dim() != 2 or pm.dtype != torch.float64 or not pm.is_cuda or pm.stride(1) != 1 or pm.shape[1] < 1:
        raise RuntimeError("pm must be a float64 device matrix [nvar, K] with contiguous rows.")
    return pm.shape[0], pm.shape[1]


def hipConvTokenSubstProj(tokens, table, pm, b, out, radem, chi, seqlen, conv_width, scaling_type, fit_intercept, slab_rows=0,
                          workspace=None):
    """``out[n, L, V, K]`` (float64, OVERWRITTEN) <- ``z'^T pm`` over the first ``nvar = pm.shape[0]`` feature columns z' of the
    sequence with token l replaced by v, for every position l and token v of the sequence and graph kernels
    (include/xgpr_hip/edit_proj.h): ``b[i]`` bit for bit at a sequence's own token, exactly 0.0 past its length.  ``pm`` float64
    [nvar, K] (rows may be strided; nvar even), ``b`` [n, K] = the sequences' columns times pm, float64 and precomputed by the
    caller.  ``slab_rows`` as for hipConvTokenSubstVarScan.  Shapes for which ``conv_token_edit_proj_ok`` is 0 raise RuntimeError
    and launch nothing."""
    t, tab = _dev(tokens, "tokens", torch.uint8, 2), _dev(table, "table", torch.float32, 2)
    r, c = _radem3(radem), _dev(chi, "chi", torch.float32, 1)
    g = _dev(out, "out", torch.float64, 4)
    n, L = tokens.shape
    nvar, K = _proj_matrix(pm)
    bb = _dev(b, "b", torch.float64, 2)
    if tuple(out.shape) != (n, L, table.shape[0], K) or tuple(b.shape) != (n, K):
        raise RuntimeError("Wrong array sizes.")
    host, dev, slab_rows, ws, wp, wn = _var_scan_workspace(tokens, radem, seqlen, nvar, n * L * table.shape[0], slab_rows, workspace,
                                                           conv_token_edit_proj_workspace_bytes)
    return _lib.check(_LIB.xgpr_conv_token_subst_proj_f32(
        t, tab, C.c_void_p(pm.data_ptr()), pm.stride(0), bb, g, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L,
        table.shape[0], table.shape[1], chi.shape[0], radem.shape[2], nvar, K, int(conv_width), int(scaling_type),
        int(bool(fit_intercept)), int(slab_rows), wp, wn, _stream()))


def hipConvTokenIndelProj(tokens, table, pm, b_del, b_ins, deletions, insertions, radem, chi, seqlen, conv_width, scaling_type,
                          fit_intercept, slab_rows=0, workspace=None):
    """``deletions[n, L, K]`` <- ``z'^T pm`` over the first ``nvar = pm.shape[0]`` feature columns z' of the sequence without its
    token at p, and ``insertions[n, L + 1, V, K]`` <- the same for the sequence with table row v inserted before position g (g =
    length appends); both float64 and OVERWRITTEN, exactly 0.0 past a sequence's length, quiet NaN for the deletions of a
    sequence of conv_width tokens (include/xgpr_hip/edit_proj.h).  ``b_del``, ``b_ins`` [n, K] = b^T pm for the sequences'
    rescaled columns b = rho z + (1 - rho) e0 with each row set's own rho, float64 and precomputed by the caller.  Either group
    (b, output) may be None as a whole (that half is skipped), not both.  ``slab_rows`` as for hipConvTokenIndelVarScan.  Shapes
    for which ``conv_token_edit_proj_ok`` is 0 raise RuntimeError and launch nothing."""
    t, tab = _dev(tokens, "tokens", torch.uint8, 2), _dev(table, "table", torch.float32, 2)
    r, c = _radem3(radem), _dev(chi, "chi", torch.float32, 1)
    n, L = tokens.shape
    V = table.shape[0]
    nvar, K = _proj_matrix(pm)
    ptrs = []
    for b, out, shape, what in ((b_del, deletions, (n, L, K), "deletions"), (b_ins, insertions, (n, L + 1, V, K), "insertions")):
        if b is None and out is None:
            ptrs.append((None, None))
            continue
        if b is None or out is None:
            raise RuntimeError(f"{what}: b and the output are given together or not at all.")
        ptrs.append((_dev(b, "b", torch.float64, 2), _dev(out, what, torch.float64, len(shape))))
        if tuple(out.shape) != shape or tuple(b.shape) != (n, K):
            raise RuntimeError("Wrong array sizes.")
    host, dev, slab_rows, ws, wp, wn = _var_scan_workspace(tokens, radem, seqlen, nvar, n * (L + 1) * V, slab_rows, workspace,
                                                           conv_token_edit_proj_workspace_bytes)
    (bd, od), (bi, oi) = ptrs
    return _lib.check(_LIB.xgpr_conv_token_indel_proj_f32(
        t, tab, C.c_void_p(pm.data_ptr()), pm.stride(0), bd, bi, od, oi, r, c, C.c_void_p(host.ctypes.data),
        C.c_void_p(dev.data_ptr()), n, L, V, table.shape[1], chi.shape[0], radem.shape[2], nvar, K, int(conv_width),
        int(scaling_type), int(bool(fit_intercept)), int(slab_rows), wp, wn, _stream()))


def conv_maxpool_input_grad_ok(width):
    """Whether hipConvMaxpoolInputGrad's kernel serves a window of ``width`` = conv_width * C elements (padded width up to 1024)."""
    return int(_LIB.xgpr_conv_maxpool_input_grad_ok(int(width)))


def conv_token_maxpool_input_grad_ok(width, vocab, C):
    """Whether hipConvTokenMaxpoolInputGrad serves the window and holds a table of ``vocab`` rows and ``C`` columns in LDS."""
    return int(_LIB.xgpr_conv_token_maxpool_input_grad_ok(int(width), int(vocab), int(C)))


def _pool_grad_tail(g, out, argmax, shape, chi, radem, workspace, device):
    n = shape[0]
    if tuple(out.shape) != tuple(shape) or tuple(argmax.shape) != (n, chi.shape[0]):
        raise RuntimeError("Wrong array sizes.")
    stride, avail = _grad_weights(g, n)
    if avail < chi.shape[0]:
        raise RuntimeError("Wrong array sizes.")
    if workspace is None:
        ws, wp, wn = _workspace(_LIB.xgpr_rbf_workspace_bytes(radem.shape[2]), device)
    else:
        ws, wp, wn = workspace, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel() * workspace.element_size())
    return stride, ws, wp, wn


def hipConvMaxpoolInputGrad(x, g, out, argmax, radem, chi, seqlen, conv_width, workspace=None):
    """``out[n, L, C]`` (float64, OVERWRITTEN; exactly 0.0 past a sequence's length) <- d m / d x through the first layer of the
    two-layer kernel, for ``g[i, f]`` = d m / d (hipConv1dMaxpool's pooled value f of sequence i)
    (include/xgpr_hip_pool_input_grad.h).  ``x`` [n, L, C] float32 UNSCALED; ``g`` float64, one vector [>= F] for all sequences or
    [n, stride >= F]; ``argmax`` int32 [n, F] (OVERWRITTEN): the first k-mer that attains each filter's maximum, -1 where the
    maximum is <= 0; ``seqlen`` int32 on the host."""
    xp = _dev(x, "x", torch.float32, 3)
    o = _dev(out, "out", torch.float64, 3)
    am = _dev(argmax, "argmax", torch.int32, 2)
    r = _radem3(radem)
    c = _dev(chi, "chi", torch.float32, 1)
    n, L, ch = x.shape
    host, dev = _seqlens(seqlen, x.device)
    if host.shape[0] != n:
        raise RuntimeError("wrong array sizes")
    stride, ws, wp, wn = _pool_grad_tail(g, out, argmax, (n, L, ch), chi, radem, workspace, x.device)
    return _lib.check(_LIB.xgpr_conv_maxpool_input_grad_f32(
        xp, C.c_void_p(g.data_ptr()), o, am, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L, ch, stride,
        chi.shape[0], radem.shape[2], int(conv_width), wp, wn, _stream()))


def hipConvTokenMaxpoolInputGrad(tokens, table, g, out, argmax, radem, chi, seqlen, conv_width, workspace=None):
    """hipConvMaxpoolInputGrad for sequences given as tokens: ``tokens`` [n, L] uint8 index the rows of ``table`` [V, C] float32
    (unscaled); ``out`` and ``argmax`` receive exactly what hipConvMaxpoolInputGrad writes for ``table[tokens]``.  Shapes for which
    ``conv_token_maxpool_input_grad_ok`` is 0 raise RuntimeError and launch nothing."""
    t = _dev(tokens, "tokens", torch.uint8, 2)
    tab = _dev(table, "table", torch.float32, 2)
    o = _dev(out, "out", torch.float64, 3)
    am = _dev(argmax, "argmax", torch.int32, 2)
    r = _radem3(radem)
    c = _dev(chi, "chi", torch.float32, 1)
    n, L = tokens.shape
    host, dev = _seqlens(seqlen, tokens.device)
    if host.shape[0] != n:
        raise RuntimeError("wrong array sizes")
    stride, ws, wp, wn = _pool_grad_tail(g, out, argmax, (n, L, table.shape[1]), chi, radem, workspace, tokens.device)
    return _lib.check(_LIB.xgpr_conv_token_maxpool_input_grad_f32(
        t, tab, C.c_void_p(g.data_ptr()), o, am, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr()), n, L,
        table.shape[0], table.shape[1], stride, chi.shape[0], radem.shape[2], int(conv_width), wp, wn, _stream()))


POOL_EDIT_MODES = {"deletions": 1, "insertions": 2, "substitutions": 3}      # include/xgpr_hip/pool_edits.h XGPR_POOL_EDIT_*


def conv_token_maxpool_edits_ok(width, vocab, C, num_rffs):
    """Whether hipConvTokenMaxpoolTables / hipConvTokenMaxpoolEdits serve a window of ``width`` = conv_width * C elements over a
    table of ``vocab`` rows and ``C`` columns with ``num_rffs`` filters (the shapes of ``conv_token_maxpool_input_grad_ok``)."""
    return int(_LIB.xgpr_conv_token_maxpool_edits_ok(int(width), int(vocab), int(C), int(num_rffs)))


def _pool_edit_operands(tokens, table, pm, sm, radem, chi, seqlen, conv_width, workspace):
    t = _dev(tokens, "tokens", torch.uint8, 2)
    tab = _dev(table, "table", torch.float32, 2)
    p = _dev(pm, "pm", torch.float32, 3)
    s = _dev(sm, "sm", torch.float32, 3)
    r = _radem3(radem)
    c = _dev(chi, "chi", torch.float32, 1)
    n, L = tokens.shape
    host, dev = _seqlens(seqlen, tokens.device)
    rows = (n, L - int(conv_width) + 2, chi.shape[0])
    if tuple(pm.shape) != rows or tuple(sm.shape) != rows:
        raise RuntimeError("Wrong array sizes.")
    if workspace is None:
        ws, wp, wn = _workspace(_LIB.xgpr_rbf_workspace_bytes(radem.shape[2]), tokens.device)
    else:
        ws, wp, wn = workspace, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel() * workspace.element_size())
    return (t, tab, p, s, r, c, C.c_void_p(host.ctypes.data), C.c_void_p(dev.data_ptr())), host, ws, wp, wn


def hipConvTokenMaxpoolTables(tokens, table, pm, sm, radem, chi, seqlen, conv_width, workspace=None):
    """``pm``, ``sm`` [n, L - conv_width + 2, F] float32 (both OVERWRITTEN as a whole) <- the prefix and suffix maxima of the
    max-pool operator's projections over the k-mer windows of ``table[tokens]`` (include/xgpr_hip/pool_edits.h): ``pm[i, j]`` is what
    hipConvTokenMaxpool leaves in a zeroed row for the first j windows of sequence i, ``sm[i, j]`` for the windows from j on; rows
    past a sequence's window count are exact zeros.  ``tokens`` [n, L] uint8, ``table`` [V, C] float32 UNSCALED, ``seqlen`` int32
    on the host.  Shapes for which ``conv_token_maxpool_edits_ok`` is 0 raise RuntimeError and launch nothing."""
    ops, host, ws, wp, wn = _pool_edit_operands(tokens, table, pm, sm, radem, chi, seqlen, conv_width, workspace)
    t, tab, p, s, r, c, hp, dp = ops
    return _lib.check(_LIB.xgpr_conv_token_maxpool_tables_f32(
        t, tab, p, s, r, c, hp, dp, tokens.shape[0], tokens.shape[1], table.shape[0], table.shape[1], chi.shape[0], radem.shape[2],
        host.shape[0], int(conv_width), wp, wn, _stream()))


def hipConvTokenMaxpoolEdits(tokens, table, pm, sm, out, radem, chi, seqlen, conv_width, mode, slot_lo, nslots, workspace=None):
    """``out`` (float32, OVERWRITTEN) <- the pooled first-layer row of every single-token mutant in the slots
    [slot_lo, slot_lo + nslots) of the flattened (sequence, slot) index, from the tables of hipConvTokenMaxpoolTables and about
    conv_width new windows per mutant; no mutant is written.  ``mode`` "substitutions": slot = position l of L, ``out``
    [nslots, V, F]; "deletions": slot = position p of L, ``out`` [nslots, F] (NaN rows for a sequence of exactly conv_width
    tokens); "insertions": slot = gap g of L + 1 (g = the length appends), ``out`` [nslots, V, F].  Slots past a sequence are
    exact zero rows.  Every value equals what hipConvTokenMaxpool leaves in a zeroed row for the written-out mutant, bit for bit
    wherever it is not zero; the sign of a zero is unspecified."""
    if mode not in POOL_EDIT_MODES:
        raise RuntimeError("mode must be one of 'substitutions', 'deletions', 'insertions'.")
    ops, host, ws, wp, wn = _pool_edit_operands(tokens, table, pm, sm, radem, chi, seqlen, conv_width, workspace)
    t, tab, p, s, r, c, hp, dp = ops
    F, V = chi.shape[0], table.shape[0]
    shape = (int(nslots), F) if mode == "deletions" else (int(nslots), V, F)
    if isinstance(out, torch.Tensor) and tuple(out.shape) != shape:
        raise RuntimeError("Wrong array sizes.")
    o = _dev(out, "out", torch.float32, len(shape))
    return _lib.check(_LIB.xgpr_conv_token_maxpool_edits_f32(
        t, tab, p, s, o, r, c, hp, dp, tokens.shape[0], tokens.shape[1], V, table.shape[1], F, radem.shape[2], host.shape[0],
        int(conv_width), POOL_EDIT_MODES[mode], int(slot_lo), int(nslots), wp, wn, _stream()))


def kmeans_ok(num_rffs, k):
    """Whether hipKMeansAssign / hipKMeansUpdate serve ``k`` centres over rows of ``num_rffs`` columns (a multiple of 4, at
    most 256 centres)."""
    return int(_LIB.xgpr_kmeans_ok(int(num_rffs), int(k)))


def _kmeans_ws(need, workspace, device):
    if workspace is None:
        return _workspace(need, device) if need else (None, None, C.c_size_t(0))
    return workspace, C.c_void_p(workspace.data_ptr()), C.c_size_t(workspace.numel() * workspace.element_size())


def hipKMeansAssign(rows, centers, labels, dist2=None, workspace=None):
    """``labels[i]`` (int32 [n], OVERWRITTEN) <- the lowest k that minimises ``|c_k|^2 - 2 rows[i] . c_k`` over the centres
    ``centers`` [K, num_rffs] float64, for float32 rows taken as they are (include/xgpr_hip_cluster.h); ``dist2`` (float64 [n],
    optional, OVERWRITTEN) <- the squared distance to that centre.  Float64 products and sums on the matrix cores, a fixed
    order.  Shapes for which ``kmeans_ok`` is 0 raise RuntimeError and launch nothing."""
    z = _dev(rows, "rows", torch.float32, 2)
    c = _dev(centers, "centers", torch.float64, 2)
    lab = _dev(labels, "labels", torch.int32, 1)
    d = None if dist2 is None else _dev(dist2, "dist2", torch.float64, 1)
    n, m = rows.shape
    k = centers.shape[0]
    if centers.shape[1] != m or labels.shape[0] != n or (dist2 is not None and dist2.shape[0] != n):
        raise RuntimeError("Wrong array sizes.")
    ws, wp, wn = _kmeans_ws(int(_LIB.xgpr_kmeans_assign_workspace_bytes(n, m, k)), workspace, rows.device)
    return _lib.check(_LIB.xgpr_kmeans_assign_f32(z, c, lab, d, n, m, k, wp, wn, _stream()))


def hipKMeansUpdate(rows, labels, sums, counts, accumulate=False, workspace=None):
    """``sums[k]`` (float64 [K, num_rffs]) (+)= the sum of the float32 rows that carry label k, ``counts[k]`` (int64 [K]) (+)=
    their number; labels outside [0, K) are skipped.  ``accumulate`` False: both arrays are OVERWRITTEN as a whole (zeros for an
    empty cluster).  No atomics on floating-point values: a fixed order.  Shapes for which ``kmeans_ok`` is 0 raise RuntimeError
    and launch nothing."""
    z = _dev(rows, "rows", torch.float32, 2)
    lab = _dev(labels, "labels", torch.int32, 1)
    s = _dev(sums, "sums", torch.float64, 2)
    cnt = _dev(counts, "counts", torch.int64, 1)
    n, m = rows.shape
    k = sums.shape[0]
    if sums.shape[1] != m or labels.shape[0] != n or counts.shape[0] != k:
        raise RuntimeError("Wrong array sizes.")
    ws, wp, wn = _kmeans_ws(int(_LIB.xgpr_kmeans_update_workspace_bytes(n, m, k)), workspace, rows.device)
    return _lib.check(_LIB.xgpr_kmeans_update_f32(z, lab, s, cnt, n, m, k, int(bool(accumulate)), wp, wn, _stream()))


def selftest_lane_xor(device="cuda"):
    """Runs the cross-lane butterfly self test; returns an int32 [6, 16, 64] CPU array."""
    out = torch.zeros(6 * 16 * 64, dtype=torch.int32, device=device)
    _lib.check(_LIB.xgpr_selftest_lane_xor(C.c_void_p(out.data_ptr()), _stream()))
    return out.cpu().numpy().reshape(6, 16, 64)


# the reference's names, so that its kernel classes / tests can bind to this module unchanged
cudaFastHadamardTransform2D = hipFastHadamardTransform2D
cudaSRHT = hipSRHT
cudaRBFFeatureGen = hipRBFFeatureGen
cudaRBFGrad = hipRBFGrad
cudaMiniARDGrad = hipMiniARDGrad
cudaConv1dMaxpool = hipConv1dMaxpool
cudaConv1dFGen = hipConv1dFGen
cudaConvGrad = hipConvGrad
cudaConvTokenRows = hipConvTokenRows
cudaConvTokenGradRows = hipConvTokenGradRows
cudaConvTokenMaxpool = hipConvTokenMaxpool
cudaRowsToHalf = hipRowsToHalf
cudaZCacheMatvecHalf = hipZCacheMatvecHalf
cudaZCacheMatvecHalfScaled = hipZCacheMatvecHalfScaled
