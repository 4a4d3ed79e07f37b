"""Submap ingest: the reference reads every cloud with np.fromfile as 4096 x 3 float64, stacks a
batch, converts with `.float()` and moves it with `.to(device)` on the step's own stream (loading_pointclouds.py:26-47,
evaluate.py:111-117).  Here the raw float64 bytes are read into pinned host buffers, copied on a side HIP stream while the
previous batch is being embedded, and narrowed to float32 on the GPU (lpd_f64_to_f32): the forward never waits for the
host, and the host does no per-element work.

  load_pc_file / load_pc_files   loading_pointclouds.py:26-47, same return values (numpy float64)
  SubmapStream                   iterator over device batches [B,1,N,3] float32, double-buffered
  get_latent_vectors_from_files  evaluate.get_latent_vectors on a list of file names
  load_scan_file / ScanStream / get_latent_vectors_from_scans
                                 the same for RAW scans of any length (no counterpart in the reference): rows of float64 xyz or
                                 KITTI-style float32 x 4, made into submaps on the device (submap.make_submaps)
  evaluate_model_from_sets       evaluate.evaluate_model on the reference's pickled DATABASE_SETS / QUERY_SETS
  load_poses                     a KITTI-style poses file (twelve numbers per line) -> [S, 12] float64, for lpdnet_hip.drive
"""
import os

import numpy as np
import torch

from . import ops

NUM_POINTS = 4096


def load_pc_file(filename, dataset_folder="", num_points=NUM_POINTS):
    """-> [num_points, 3] float64, or an empty array when the file does not hold num_points * 3 doubles (the reference logs
    "Error in pointcloud shape" and returns np.array([]))."""
    pc = np.fromfile(os.path.join(dataset_folder, filename), dtype=np.float64)
    if pc.shape[0] != num_points * 3:
        return np.array([])
    return np.reshape(pc, (pc.shape[0] // 3, 3))


def load_pc_files(filenames, dataset_folder="", num_points=NUM_POINTS):
    """-> [n_ok, num_points, 3] float64; files of the wrong size are skipped (loading_pointclouds.py:38-47)."""
    pcs = []
    for filename in filenames:
        pc = load_pc_file(filename, dataset_folder, num_points)
        if pc.shape[0] != num_points:
            continue
        pcs.append(pc)
    return np.array(pcs)


class SubmapStream:
    """for batch in SubmapStream(files, 32, folder, device): batch is a float32 CUDA tensor [b,1,N,3] on the CURRENT stream
    (b <= batch_size: ragged tail, wrong-size files skipped like load_pc_files).  Two pinned buffers and a copy stream:
    batch i+1 is read from disk and copied while batch i is consumed."""

    def __init__(self, filenames, batch_size, dataset_folder="", device=None, num_points=NUM_POINTS):
        self.files = list(filenames)
        self.bs, self.folder, self.N = int(batch_size), dataset_folder, int(num_points)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.pinned = [torch.empty((self.bs, self.N, 3), dtype=torch.float64).pin_memory() for _ in range(2)]
        self.staged = [torch.empty((self.bs, self.N, 3), dtype=torch.float64, device=self.device) for _ in range(2)]
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]     # H2D copy of slot s finished
        self.free = [torch.cuda.Event(), torch.cuda.Event()]      # consumer finished reading slot s

    def _stage(self, slot, start):
        """read up to batch_size valid clouds starting at file index `start` into slot; -> (count, next file index)"""
        self.ready[slot].synchronize()        # the previous H2D copy out of this pinned buffer has left the host
        host = self.pinned[slot].numpy()
        n, i = 0, start
        while n < self.bs and i < len(self.files):
            pc = np.fromfile(os.path.join(self.folder, self.files[i]), dtype=np.float64)
            i += 1
            if pc.shape[0] != self.N * 3:
                continue
            host[n] = pc.reshape(self.N, 3)
            n += 1
        if n:
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(self.free[slot])          # the consumer of this device slot is done with it
                self.staged[slot][:n].copy_(self.pinned[slot][:n], non_blocking=True)
                self.ready[slot].record(self.copy_stream)
        return n, i

    def __iter__(self):
        main = torch.cuda.current_stream(self.device)
        for ev in self.free:
            ev.record(main)
        slot, pos = 0, 0
        n, pos = self._stage(slot, pos)
        while n:
            other = slot ^ 1
            n_next, pos = self._stage(other, pos) if pos < len(self.files) else (0, pos)   # disk + PCIe under the consumer
            main.wait_event(self.ready[slot])
            batch = ops.f64_to_f32(self.staged[slot][:n]).view(n, 1, self.N, 3)
            self.free[slot].record(main)
            yield batch
            slot, n = other, n_next


def get_latent_vectors_from_files(model, filenames, batch_size, dataset_folder="", output_dim=256, num_points=NUM_POINTS):
    """evaluate.py:96-159 on file names: eval mode, no_grad, batches of `batch_size` clouds streamed from disk, the previous
    train/eval mode restored afterwards (like harness.get_latent_vectors); -> numpy [n_ok, output_dim]."""
    was_training = model.training
    model.eval()
    outs = []
    dev = next(model.parameters()).device
    try:
        with torch.no_grad():
            for batch in SubmapStream(filenames, batch_size, dataset_folder, dev, num_points):
                outs.append(model(batch).detach().cpu().numpy().reshape(batch.shape[0], -1))
    finally:
        model.train(was_training)
    return np.concatenate(outs, 0) if outs else np.zeros((0, output_dim), np.float32)


def load_scan_file(filename, dataset_folder="", dtype=np.float64, columns=3):
    """A raw scan of any length: -> [n, columns] of `dtype` (the first three columns are the coordinates; KITTI velodyne files are
    dtype=np.float32, columns=4), or an empty array when the file is empty or not a whole number of rows."""
    pc = np.fromfile(os.path.join(dataset_folder, filename), dtype=dtype)
    if columns < 3 or pc.shape[0] == 0 or pc.shape[0] % columns:
        return np.array([])
    return np.reshape(pc, (pc.shape[0] // columns, columns))


def load_poses(path, dataset_folder=""):
    """A KITTI-style poses file -- one scan per line, twelve numbers: the top three rows of the sensor-to-world matrix, row-major --
    -> [S, 12] float64, what drive.plan_windows / accumulate / submaps_from_drive take.  Blank lines and lines that start with `#` are
    skipped; any other line that does not hold twelve numbers raises ValueError with its line number."""
    rows = []
    with open(os.path.join(dataset_folder, path)) as fh:
        for no, line in enumerate(fh, 1):
            text = line.strip()
            if not text or text.startswith("#"):
                continue
            fields = text.replace(",", " ").split()
            try:
                vals = [float(f) for f in fields]
            except ValueError:
                raise ValueError(f"{path}:{no}: not a number in {text[:60]!r}") from None
            if len(vals) != 12:
                raise ValueError(f"{path}:{no}: {len(vals)} numbers, a pose line holds 12")
            rows.append(vals)
    if not rows:
        raise ValueError(f"{path}: no poses")
    return np.asarray(rows, dtype=np.float64)


class ScanStream:
    """The ragged sibling of SubmapStream: for batch in ScanStream(files, 32, folder, device): batch is a float32 CUDA tensor
    [b,1,N,3] of submaps made on the device from b raw scans of any length (submap.make_submaps; `last` holds the whole result of
    the batch just yielded).  Files are rows of `columns` values of `dtype`; a file that is empty, not a whole number of rows or
    longer than 2^20 rows is skipped.  Two pinned byte buffers and a copy stream, as SubmapStream; the buffers are sized from the
    byte sizes of the first batch's files and grow when a later batch needs more.  float64 rows are narrowed on the device
    (lpd_f64_to_f32); float32 rows go to the kernel as they are, with ld = columns.  clean: a submap.RoadRemoval -- range crop and
    road removal on the device in front of the submaps (submap.make_submaps(clean=...); `last.cleaned` holds what it did)."""

    def __init__(self, filenames, batch_size, dataset_folder="", device=None, num_points=NUM_POINTS, dtype=np.float64, columns=3,
                 normalize=True, clean=None):
        self.files = list(filenames)
        self.clean = clean
        self.bs, self.folder, self.N = int(batch_size), dataset_folder, int(num_points)
        self.dtype, self.columns, self.normalize = np.dtype(dtype), int(columns), bool(normalize)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)) or self.columns < 3:
            raise ValueError(f"ScanStream: rows of >= 3 float64 or float32 values, got {self.columns} x {self.dtype}")
        if not ops.SUBMAP_MIN_N <= self.N <= ops.SUBMAP_MAX_N:
            raise ValueError(f"ScanStream: num_points={self.N} outside {ops.SUBMAP_MIN_N} .. {ops.SUBMAP_MAX_N}")
        self.row_bytes = self.columns * self.dtype.itemsize
        self.device = device
        first = sum(self._file_bytes(f) for f in self.files[:self.bs])
        self.host = [self._host_buffer(max(first, self.row_bytes)) for _ in range(2)]
        self.staged = [None, None]
        self.grown = 0            # how often a host buffer had to grow
        self.last = None

    def _file_bytes(self, f):
        try:
            return os.path.getsize(os.path.join(self.folder, f))
        except OSError:
            return 0

    @staticmethod
    def _host_buffer(nbytes):
        buf = torch.empty((int(nbytes),), dtype=torch.uint8)
        return buf.pin_memory() if torch.cuda.is_available() else buf

    def _read(self, slot, start):
        """read up to batch_size valid scans starting at file index `start` into host buffer `slot`, growing it when the files need
        more; -> (lengths, next file index).  Host work only."""
        lengths, used, i = [], 0, start
        while len(lengths) < self.bs and i < len(self.files):
            path = os.path.join(self.folder, self.files[i])
            i += 1
            nbytes = self._file_bytes(self.files[i - 1])
            rows = nbytes // self.row_bytes
            if nbytes == 0 or nbytes % self.row_bytes or rows > ops.SUBMAP_MAX_POINTS:
                continue
            if used + nbytes > self.host[slot].numel():
                bigger = self._host_buffer(max(used + nbytes, self.host[slot].numel() * 3 // 2))
                bigger[:used] = self.host[slot][:used]
                self.host[slot] = bigger
                self.grown += 1
            with open(path, "rb") as fh:
                got = fh.readinto(memoryview(self.host[slot].numpy())[used:used + nbytes])
            if got != nbytes:
                continue
            lengths.append(rows)
            used += nbytes
        return lengths, i

    def _stage(self, slot, start):
        self.ready[slot].synchronize()        # the previous H2D copy out of this pinned buffer has left the host
        lengths, i = self._read(slot, start)
        if lengths:
            used = sum(lengths) * self.row_bytes
            if self.staged[slot] is None or self.staged[slot].numel() < used:
                self.free[slot].synchronize()     # nobody reads the old device buffer any more
                self.staged[slot] = torch.empty((max(used, self.host[slot].numel()),), dtype=torch.uint8, device=self.device)
                self.free[slot].record(self.main)     # whatever used this memory before was enqueued on the main stream before now
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(self.free[slot])
                self.staged[slot][:used].copy_(self.host[slot][:used], non_blocking=True)
                self.ready[slot].record(self.copy_stream)
        return lengths, i

    def __iter__(self):
        from . import submap
        self.device = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]
        self.free = [torch.cuda.Event(), torch.cuda.Event()]
        self.main = main = torch.cuda.current_stream(self.device)
        for ev in self.free:
            ev.record(main)
        tdtype = torch.float64 if self.dtype == np.dtype(np.float64) else torch.float32
        slot, pos = 0, 0
        lengths, pos = self._stage(slot, pos)
        while lengths:
            other = slot ^ 1
            nxt, pos = self._stage(other, pos) if pos < len(self.files) else ([], pos)
            main.wait_event(self.ready[slot])
            rows = self.staged[slot][:sum(lengths) * self.row_bytes].view(tdtype).view(-1, self.columns)
            self.last = submap.make_submaps(rows, lengths, self.N, self.normalize, check_finite=False, clean=self.clean)
            self.free[slot].record(main)
            yield self.last.x
            slot, lengths = other, nxt


def get_latent_vectors_from_scans(model, filenames, batch_size, dataset_folder="", output_dim=256, num_points=NUM_POINTS,
                                  dtype=np.float64, columns=3, normalize=True, clean=None):
    """get_latent_vectors_from_files for raw scans of any length: eval mode, no_grad, batches of `batch_size` scans streamed from
    disk and made into submaps on the device (ScanStream), ragged tail, the previous train/eval mode restored afterwards;
    clean: a submap.RoadRemoval (range crop and road removal in front of the submaps) or None;  -> numpy [n_ok, output_dim]."""
    was_training = model.training
    model.eval()
    outs = []
    dev = next(model.parameters()).device
    try:
        with torch.no_grad():
            for batch in ScanStream(filenames, batch_size, dataset_folder, dev, num_points, dtype, columns, normalize, clean):
                outs.append(model(batch).detach().cpu().numpy().reshape(batch.shape[0], -1))
    finally:
        model.train(was_training)
    return np.concatenate(outs, 0) if outs else np.zeros((0, output_dim), np.float32)


def evaluate_model_from_sets(model, DATABASE_SETS, QUERY_SETS, batch_size, dataset_folder="", num_points=NUM_POINTS):
    """evaluate.evaluate_model (evaluate.py:33-93) on the reference's pickled structures: DATABASE_SETS[r][i]["query"] and
    QUERY_SETS[n][i]["query"] are submap file names (relative to dataset_folder), QUERY_SETS[n][i][m] the true neighbours of query i
    of run n in run m.  Every run is streamed from disk through SubmapStream into the embedding pipeline and kept on the device as one
    table; all (m, n) pairs, m != n, are scored in one lpd_recall_pairs launch (harness.evaluate_from_descriptors).
    -> (ave_recall, average_similarity_score, ave_one_percent_recall); the model is left in train mode.

    Files of the wrong size are skipped, exactly as load_pc_files skips them: the run's later descriptors then move up by one row,
    while the truth lists still count the pickle's rows -- the reference's own indices shift the same way.  A run with no valid file
    raises ValueError; edge cases otherwise as harness.evaluate_pairs."""
    from . import harness
    harness._cuda_device_or_raise("evaluate_model_from_sets")
    dev = next(model.parameters()).device

    def embed(sets, what):
        tables, counts = [], []
        for r, run in enumerate(sets):
            files = [run[i]["query"] for i in range(len(run))]
            outs = harness._embed_batches(model, SubmapStream(files, batch_size, dataset_folder, dev, num_points), dev)
            n = sum(o.shape[0] for o in outs)
            if n == 0:
                raise ValueError(f"evaluate_model_from_sets: {what} run {r} has no submap of {num_points} points")
            tables += [o.reshape(o.shape[0], -1) for o in outs]
            counts.append(n)
        off = np.zeros(len(counts) + 1, dtype=np.int64)
        np.cumsum(counts, out=off[1:])
        return torch.cat(tables, 0).float(), off

    try:
        db = embed(DATABASE_SETS, "database")
        qv = embed(QUERY_SETS, "query")
    finally:
        model.train()
    return harness.evaluate_from_descriptors(db, qv, QUERY_SETS)
