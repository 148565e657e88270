"""k-nearest-neighbour queries over point clouds on the GPU (gsgen_amd/csrc/knn.hip through the C ABI).

The reference takes these from pytorch3d's `knn_points` (utils/ops.py:104-134) and from faiss (utils/initialize.py:16-35); neither
exists for ROCm.  The functions below keep the reference's call signatures and results.  They take CUDA (HIP) tensors and run on
the current stream. The workspace comes from torch's caching allocator. They record no autograd graph and do not synchronise with
the host, so a call can be captured by `torch.cuda.graph` and replayed on new point values in the same tensor.  The exception is
nearest_neighbor_initialize, which returns its result on the CPU as the reference does.

With `query=None` every point is also a query (the self search); with a `[Q,3]` query tensor row q lists the neighbours of
query[q] among `points` (gsgen_knn_query), d = p_j - q.

Neighbour order: ascending squared distance, ties by ascending index.  In the self search each point is its own first neighbour
unless a lower-index exact duplicate of it exists.  A non-finite query's row is all (-1, +inf).  A point with a NaN / Inf coordinate is nobody's neighbour; its row, and any row short of K finite
points, holds index -1 and distance +inf.
"""
import numpy as np
import torch

from . import _capi

K_MAX = 32


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "knn"):
        raise RuntimeError(f"{lib.path} was built without the kNN kernel (gsgen_amd/csrc/knn.hip): rebuild it (python -m gsgen_amd.build)")
    return lib


def _check_points(points, K):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"gsgen_amd.knn: points must be a [N, 3] tensor, got {getattr(points, 'shape', type(points))}")
    N = points.shape[0]
    if not 1 <= K <= K_MAX:
        raise ValueError(f"gsgen_amd.knn: K = {K} is not in 1..{K_MAX}")
    if N == 0 or K > N:
        raise ValueError(f"gsgen_amd.knn: K = {K} neighbours of {N} points")
    if not points.is_cuda:
        raise ValueError("gsgen_amd.knn: points must be a CUDA (HIP) tensor -- there is no CPU implementation")
    return N


def _check_query(points, query):
    if not isinstance(query, torch.Tensor) or query.dim() != 2 or query.shape[1] != 3:
        raise ValueError(f"gsgen_amd.knn: query must be a [Q, 3] tensor, got {getattr(query, 'shape', type(query))}")
    if not query.is_cuda:
        raise NotImplementedError("gsgen_amd.knn: a query set on the CPU -- there is no CPU implementation of the query search")
    if query.device != points.device:
        raise ValueError("gsgen_amd.knn: query must be on the device of points")
    return query.shape[0]


@torch.no_grad()
def knn_raw(points, K, query=None):
    """-> (dist2 [N,K] float32, idx [N,K] int32): the kernel's own output; with query [Q,3]: [Q,K], the neighbours of each query"""
    K = int(K)
    Q = _check_query(points, query) if query is not None else None
    N = _check_points(points, K)
    pts = points.detach().to(torch.float32).contiguous()
    dev = pts.device
    lib = _lib()
    if query is not None:
        if not hasattr(lib, "knn_query"):
            raise RuntimeError(f"{lib.path} was built without gsgen_knn_query: rebuild it (python -m gsgen_amd.build)")
        qs = query.detach().to(torch.float32).contiguous()
        dist2 = torch.empty(Q, K, device=dev, dtype=torch.float32)
        idx = torch.empty(Q, K, device=dev, dtype=torch.int32)
        nbytes = lib.knn_query_workspace_bytes(N, Q, K)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        lib.knn_query(pts.data_ptr(), N, qs.data_ptr(), Q, K, dist2.data_ptr(), idx.data_ptr(), ws.data_ptr(), nbytes,
                      torch.cuda.current_stream(dev).cuda_stream)
        return dist2, idx
    dist2 = torch.empty(N, K, device=dev, dtype=torch.float32)
    idx = torch.empty(N, K, device=dev, dtype=torch.int32)
    nbytes = lib.knn_workspace_bytes(N, K)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    lib.knn(pts.data_ptr(), N, K, dist2.data_ptr(), idx.data_ptr(), ws.data_ptr(), nbytes,
            torch.cuda.current_stream(dev).cuda_stream)
    return dist2, idx


@torch.no_grad()
def knn_points(points, K, query=None):
    """self kNN of points [N,3] -> (dist2 [N,K] float32, squared distances; idx [N,K] int64), pytorch3d's knn_points(p[None],
    p[None], K) without the batch axis; with query [Q,3]: knn_points(query[None], p[None], K), [Q,K]"""
    dist2, idx = knn_raw(points, K, query)
    return dist2, idx.long()


@torch.no_grad()
def nearest_neighbor(mean):
    """utils/ops.py:104-114: column 1 of a K = 2 search -> (position of each point's nearest other point [N,3], its index [N])"""
    _, idx = knn_points(mean, 2)
    nn_idx = idx[:, 1]
    return mean.detach()[nn_idx], nn_idx


@torch.no_grad()
def K_nearest_neighbors(mean, K, query=None, return_dist=False):
    """utils/ops.py:117-134: a K search with column 0 (the point itself) dropped -> (nn [N,K-1,3], idx [N,K-1](, dist2 [N,K-1])).
    With query [Q,3] the rows are the queries' ([Q,K-1,...]) and column 0 -- then the query's NEAREST point, not the query -- is
    dropped all the same: that is the reference's behaviour (utils/ops.py:129-134 slices [1:] whatever the query set is, and its
    density grid, utils/export.py:94-96, relies on it), not an oversight of this port."""
    dist2, idx = knn_points(mean, K, query)
    idx = idx[:, 1:]
    nn = mean.detach()[idx]
    return (nn, idx, dist2[:, 1:]) if return_dist else (nn, idx)


@torch.no_grad()
def nearest_neighbor_initialize(pts, k=3):
    """utils/initialize.py:16-35: the mean squared distance of every point to its k nearest other points (faiss IndexFlatL2
    returns squared distances) -> [N] float32 on the CPU, as the reference returns it (an initialiser: its one copy back is
    the only host synchronisation in this module).  A numpy array is searched on the current CUDA device."""
    t = pts if isinstance(pts, torch.Tensor) else torch.as_tensor(np.asarray(pts, np.float32)).cuda()
    dist2, _ = knn_raw(t, int(k) + 1)
    return dist2[:, 1:].mean(dim=1).cpu()
