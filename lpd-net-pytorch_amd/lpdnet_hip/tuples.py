"""Training tuples on the device: the cloud table of the whole training set and its positive / near lists stay in HBM, and a
training batch is a few small launches (lpd_sample_items, lpd_gather_tuples; definitions in include/lpd_hip.h).  Only item numbers
cross the bus.

Replaces what the reference's Dataset.__getitem__ does per query in Python (util/data.py:56-101, 190-271; loading_pointclouds.py:
50-142): shuffle of the `negatives` list, the set difference for `other_neg`, fancy-indexing 22 float64 clouds, cast, collate, copy,
and the numpy rotation / jitter.

    bank  = TupleBank.from_queries_dict(TRAINING_QUERIES, TRAINING_POINT_CLOUD)        # once, from the reference's pickle, or
    bank  = TupleBank.from_positions(TRAINING_POINT_CLOUD, positions)                  # ... from [T, 2] positions (places.py)
    items = bank.sample(query_items, P=2, Ng=18, seed=step)                             # [bq, 2 + P + Ng] int32 on the device
    feed  = bank.assemble(items, rotate=True, jitter=True, seed=step)                   # [bq * (2+P+Ng), 1, N, 3]

There is no CPU path: without a GPU the constructor raises (device="cpu" builds the host side of a bank only; its draws raise).
"""
import numpy as np
import torch

from . import ops
from ._lib import LpdHipError

_M64 = 0xFFFFFFFFFFFFFFFF
_GOLDEN64 = 0x9E3779B97F4A7C15
DRAW_POSITIVES, DRAW_NEGATIVES, DRAW_OTHER, DRAW_CANDIDATES, DRAW_JITTER = 0, 1, 2, 3, 4


def sub_seed(seed, draw):
    """The seed of draw number `draw` of a call with `seed`: (seed + (draw + 1) * 0x9E3779B97F4A7C15) mod 2^64.  Distinct draws of
    one call get distinct seeds (the multiples of an odd constant are distinct modulo 2^64)."""
    return (int(seed) + (int(draw) + 1) * _GOLDEN64) & _M64


def build_csr(lists, T, what="lists"):
    """A list of item lists -> (off int32 [len+1], idx int32 [nnz], lengths int64 [len]); every list sorted and without duplicates,
    so that the lengths are the sizes of the sets.  An item outside [0, T) raises ValueError."""
    rows = []
    for i, l in enumerate(lists):
        a = np.unique(np.asarray(l, dtype=np.int64).reshape(-1))
        if a.size and (a[0] < 0 or a[-1] >= T):
            raise ValueError(f"TupleBank: {what}[{i}] names an item outside 0 .. {T - 1}")
        rows.append(a)
    lens = np.fromiter((a.size for a in rows), dtype=np.int64, count=len(rows))
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError(f"TupleBank: {what} hold more than 2^31 entries")
    idx = np.concatenate(rows).astype(np.int32) if rows and off[-1] else np.zeros(0, dtype=np.int32)
    return off.astype(np.int32), idx, lens


def near_from_negatives(negatives, T):
    """near[i] = [0, T) \\ negatives[i]: what the reference's pickles leave implicit (their `negatives` are everything farther than
    50 m, so `near` is the 50 m ball, the item itself included)."""
    near = []
    mask = np.empty(T, dtype=bool)
    for neg in negatives:
        mask[:] = True
        neg = np.asarray(neg, dtype=np.int64).reshape(-1)
        mask[neg[(neg >= 0) & (neg < T)]] = False
        near.append(np.nonzero(mask)[0])
    return near


def run_dry_guarantee(T, max_near, max_pos, Ng, exclude_members=False):
    """Can a draw of `sample` come up short?  Decided from the list lengths alone: -> (negatives_ok, other_ok).
    Negatives: the pool of a query is [0, T) \\ near[q] (and the hard items, which take their places in the tuple), so
    T - max|near| >= Ng suffices.  Other: at most (1 + Ng) positive lists are excluded, so (1 + Ng) * max|positives| < T leaves an
    item; with exclude_members the query and the Ng negatives go as well: (1 + Ng) * (max|positives| + 1) < T."""
    neg_ok = T - int(max_near) >= int(Ng)
    per = int(max_pos) + (1 if exclude_members else 0)
    return bool(neg_ok), bool((1 + int(Ng)) * per < T)


class TupleBank:
    """The training set resident on the device: clouds [T, N, 3] (array-like, float64 or float32; uploaded in slices, float64
    narrowed on the device by ops.f64_to_f32: round to nearest even, as numpy's astype), positives[i] / near[i] lists of item numbers
    (near[i] = the items that are NOT negatives of i: the reference's r = 50 m ball, i included), kept as two device CSRs plus host
    length arrays.  device="cpu" builds the host side only (lists, lengths, the checks that need no device); every draw raises
    LpdHipError there, since the kernels have no CPU path."""

    SLICE_BYTES = 64 << 20      # host -> device slices of the cloud table

    def __init__(self, clouds, positives, near, device=None):
        self._open(clouds, device)
        if len(positives) != self.T or len(near) != self.T:
            raise ValueError(f"TupleBank: {self.T} clouds, {len(positives)} positive lists, {len(near)} near lists")
        self._set_lists(positives, near)
        self._upload(clouds)
        with self._on_device():
            self.pos_off, self.pos_idx = (torch.from_numpy(a).to(self.device) for a in self._pos_csr)
            self.near_off, self.near_idx = (torch.from_numpy(a).to(self.device) for a in self._near_csr)

    def _open(self, clouds, device):
        """the device and the shape of the cloud table: sets T, N, device"""
        if device is None and not torch.cuda.is_available():
            raise LpdHipError("TupleBank: no GPU visible; the tuple bank lives on the MI355X (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        shape = tuple(clouds.shape) if hasattr(clouds, "shape") else np.asarray(clouds).shape
        if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"TupleBank: clouds must be [T, N, 3], got {shape}")
        T, N = int(shape[0]), int(shape[1])
        if T > ops.TUPLE_MAX_ITEMS:
            raise ValueError(f"TupleBank: {T} items; at most {ops.TUPLE_MAX_ITEMS}")
        self.T, self.N, self.device = T, N, dev

    def _upload(self, clouds):
        """the cloud table, in slices"""
        T, N, dev = self.T, self.N, self.device
        self.table = torch.empty((T, N, 3), dtype=torch.float32, device=dev)
        step = max(1, self.SLICE_BYTES // (N * 3 * 8))
        with self._on_device():
            for s in range(0, T, step):
                chunk = clouds[s:s + step]
                chunk = chunk.detach().cpu().numpy() if isinstance(chunk, torch.Tensor) else np.ascontiguousarray(chunk)
                if chunk.dtype == np.float64 and dev.type == "cuda":
                    ops.f64_to_f32(torch.from_numpy(chunk).to(dev), out=self.table[s:s + step])
                else:      # float32 rows as they are (on a host-only bank torch narrows float64: the same rounding)
                    self.table[s:s + step].copy_(torch.from_numpy(chunk))

    def _on_device(self):
        import contextlib
        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    def _set_lists(self, positives, near):
        """host side of the constructor (no device): the CSRs and the length arrays"""
        po, pi, self.pos_len = build_csr(positives, self.T, "positives")
        no, ni, self.near_len = build_csr(near, self.T, "near")
        self._pos_csr, self._near_csr = (po, pi), (no, ni)
        self.max_pos = int(self.pos_len.max()) if self.T else 0
        self.max_near = int(self.near_len.max()) if self.T else 0

    @classmethod
    def from_queries_dict(cls, TRAINING_QUERIES, clouds, device=None):
        """The reference's pickle layout: {item: {'query': file, 'positives': [...], 'negatives': [...]}} with the items 0 .. T-1.
        near[i] = all \\ negatives[i] is derived once, with numpy."""
        positives, near = cls.lists_from_queries_dict(TRAINING_QUERIES)
        return cls(clouds, positives, near, device=device)

    @classmethod
    def from_positions(cls, clouds, positions, pos_radius=10.0, near_radius=50.0, device=None):
        """The bank from the items' positions [T, 2] (northing, easting; float64) instead of lists: positives[i] = the items within
        pos_radius of i without i, near[i] = the items within near_radius, made on the device (places.training_lists: what
        generate_training_tuples_baseline.py:52-60 searches with a KDTree) and installed as they are -- no Python list, no host CSR
        (`_pos_csr` / `_near_csr` are None on such a bank).  device="cpu" raises LpdHipError: the lists come from the kernel."""
        from . import places
        self = cls.__new__(cls)
        self._open(clouds, device)
        if self.device.type != "cuda":
            raise LpdHipError("TupleBank.from_positions: the place lists come from the MI355X kernel (no CPU fallback)")
        n = positions.shape[0] if hasattr(positions, "shape") else len(positions)
        if n != self.T:
            raise ValueError(f"TupleBank.from_positions: {self.T} clouds, {n} positions")
        lists = places.training_lists(positions, pos_radius, near_radius, device=self.device)
        self.pos_off, self.pos_idx, self.pos_len = lists.pos_off, lists.pos_idx, lists.pos_len
        self.near_off, self.near_idx, self.near_len = lists.near_off, lists.near_idx, lists.near_len
        self.max_pos, self.max_near = lists.max_pos, lists.max_near
        self._pos_csr = self._near_csr = None
        self._upload(clouds)
        return self

    @staticmethod
    def lists_from_queries_dict(TRAINING_QUERIES):
        T = len(TRAINING_QUERIES)
        if sorted(TRAINING_QUERIES.keys()) != list(range(T)):
            raise ValueError("TupleBank: the keys of the queries dict must be 0 .. T-1")
        positives = [TRAINING_QUERIES[i]["positives"] for i in range(T)]
        return positives, near_from_negatives([TRAINING_QUERIES[i]["negatives"] for i in range(T)], T)

    # ---- sampling -----------------------------------------------------------------------------------------------------------
    def _queries(self, query_items, what):
        q = np.asarray(query_items, dtype=np.int64).reshape(-1)
        if q.size < 1 or q.min() < 0 or q.max() >= self.T:
            raise ValueError(f"{what}: query items must be a non-empty list of numbers in 0 .. {self.T - 1}")
        return q, torch.from_numpy(q.astype(np.int32)).to(self.device, non_blocking=True)

    def _check_count(self, count, need, what, q):
        short = (count.cpu().numpy() < need)
        if short.any():
            b = int(np.argmax(short))
            raise ValueError(f"{what}: query item {int(q[b])} has a pool of fewer than {need} items")

    def sample(self, query_items, P, Ng, seed, hard=None, exclude_members=False):
        """Tuples for the queries `query_items` (host integers) -> device int32 [bq, 2 + P + Ng] in the order q, positives, negatives,
        other.
          positives  P distinct items of positives[q], uniformly
          negatives  hard[b] first (device or host [bq, H], H <= Ng), then Ng - H distinct items of [0, T) \\ near[q] that are not
                     hard: the reference's "top up from the shuffled negatives that are not hard", as a distribution
          other      one item of [0, T) \\ (positives[q] u positives[neg_1] u ... u positives[neg_Ng]): the reference's rule with
                     its quirk -- the query and the negatives themselves stay eligible unless exclude_members=True
        The three draws use sub_seed(seed, 0 / 1 / 2).  A query with fewer than P positives raises ValueError (a host length
        check, no device sync).  Whether negatives or `other` can run dry is decided from the host length arrays
        (run_dry_guarantee); only when that does not guarantee them, the pool sizes are read back from the device (one sync per
        draw) and a short pool raises ValueError."""
        P, Ng = int(P), int(Ng)
        q, q_dev = self._queries(query_items, "TupleBank.sample")
        if P < 1 or Ng < 1 or 1 + Ng > ops.TUPLE_MAX_LISTS:
            raise ValueError(f"TupleBank.sample: P={P} Ng={Ng} (P >= 1, 1 <= Ng <= {ops.TUPLE_MAX_LISTS - 1})")
        few = np.nonzero(self.pos_len[q] < P)[0]
        if few.size:
            raise ValueError(f"TupleBank.sample: query item {int(q[few[0]])} has {int(self.pos_len[q[few[0]]])} positives, {P} wanted")
        neg_ok, other_ok = run_dry_guarantee(self.T, self.max_near, self.max_pos, Ng, exclude_members)
        with self._on_device():
            qcol = q_dev.view(-1, 1)
            pos, _ = ops.sample_items(self.pos_off, self.pos_idx, self.T, qcol, None, P, 0, sub_seed(seed, DRAW_POSITIVES))
            H = 0
            if hard is not None:
                hard = torch.as_tensor(hard, dtype=torch.int32, device=self.device).reshape(q.size, -1)
                H = hard.shape[1]
                if H > Ng:
                    raise ValueError(f"TupleBank.sample: {H} hard negatives for Ng={Ng}")
            if H == Ng:
                neg = hard
            else:
                fill, cnt = ops.sample_items(self.near_off, self.near_idx, self.T, qcol, hard if H else None, Ng - H, 1,
                                             sub_seed(seed, DRAW_NEGATIVES))
                if not neg_ok:
                    self._check_count(cnt, Ng - H, "TupleBank.sample (negatives)", q)
                neg = torch.cat((hard, fill), 1) if H else fill
            members = torch.cat((qcol, neg), 1)
            other, cnt = ops.sample_items(self.pos_off, self.pos_idx, self.T, members, members if exclude_members else None, 1, 1,
                                          sub_seed(seed, DRAW_OTHER))
            if not other_ok:
                self._check_count(cnt, 1, "TupleBank.sample (other)", q)
            return torch.cat((qcol, pos, neg, other), 1)

    def candidates(self, query_items, n_sampled, seed):
        """n_sampled distinct random negatives per query (items of [0, T) \\ near[q]) -> device int32 [bq, n_sampled]; the seed of the
        draw is sub_seed(seed, 3).  A query with fewer negatives raises ValueError (read back only when T - max|near| < n_sampled)."""
        q, q_dev = self._queries(query_items, "TupleBank.candidates")
        with self._on_device():
            out, cnt = ops.sample_items(self.near_off, self.near_idx, self.T, q_dev.view(-1, 1), None, int(n_sampled), 1,
                                        sub_seed(seed, DRAW_CANDIDATES))
        if self.T - self.max_near < int(n_sampled):
            self._check_count(cnt, int(n_sampled), "TupleBank.candidates", q)
        return out

    def mine(self, latent, query_items, hard_neg_num, n_sampled=4000, seed=0, query_vecs=None):
        """Hard negatives of the queries -> device int32 [bq, hard_neg_num], nearest first: `candidates`, then ops.hard_negatives
        on the latent-vector table `latent` [T, D] (harness.update_vectors), then a gather of the positions.  query_vecs=None: the
        queries' rows of `latent`; the reference embeds the query afresh in train mode (util/data.py:236-241) -- pass such vectors
        ([bq, D]) when that matters."""
        cand = self.candidates(query_items, n_sampled, seed)
        q, q_dev = self._queries(query_items, "TupleBank.mine")
        latent = latent.to(self.device, torch.float32).contiguous()
        if query_vecs is None:
            qv = latent.index_select(0, q_dev.long())
        else:
            qv = torch.as_tensor(query_vecs, dtype=torch.float32, device=self.device).reshape(q.size, -1).contiguous()
        with self._on_device():
            pos, _ = ops.hard_negatives(latent, qv, cand, int(hard_neg_num))
        return torch.gather(cand, 1, pos.long())

    # ---- assembling ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def rotations(n, seed):
        """(cos, sin) of n angles uniform in [-pi/2, pi/2) (loading_pointclouds.py:62), from numpy.random.Generator(Philox(seed)),
        computed in float64 -> float32 [n, 2]"""
        ang = np.random.Generator(np.random.Philox(int(seed) & _M64)).random(n) * np.pi - np.pi / 2.0
        return np.stack((np.cos(ang), np.sin(ang)), 1).astype(np.float32)

    def assemble(self, items, rotate=False, jitter=False, sigma=0.005, clip=0.05, seed=0):
        """items (device int32 [bq, 2 + P + Ng] from `sample`, or any integer array) -> the model's feed [bq * (2+P+Ng), 1, N, 3] in
        one launch.  rotate: one angle per cloud about z, drawn on the host (`rotations`), shipped as one small tensor.  jitter:
        clamp(sigma * z, -clip, clip) per coordinate, z from Philox on the device with sub_seed(seed, 4)."""
        items = torch.as_tensor(items, device=self.device).to(torch.int32).reshape(-1)
        B = items.numel()
        rot = torch.from_numpy(self.rotations(B, seed)).to(self.device, non_blocking=True) if rotate else None
        out = torch.empty((B, 1, self.N, 3), dtype=torch.float32, device=self.device)
        with self._on_device():
            ops.gather_tuples(self.table, items, rot, float(sigma) if jitter else 0.0, clip, sub_seed(seed, DRAW_JITTER), out=out)
        return out
