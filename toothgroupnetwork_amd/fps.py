"""The Python front end of farthest-point sampling: one call sequence, one book and one switch for both layouts.

``sample_packed`` (pointops.fps_with_coords) and ``sample_dense`` (pointnet2_utils._fps_dense) normalise their arguments, allocate
their outputs and say what differs between them; ``_launch`` does the rest once.  This module imports only ``_lib`` and ``config``:
the packed layout's host offsets (pointops.offsets_host / register_offsets) come in as an argument.

"FPS of an FPS result is the identity" (include/tgn_pointops.h).  Every FPS launch that takes part leaves a
per-cloud certificate next to its sampled coordinates.  A later FPS call whose input has the layout of a recorded result -- the key:
("packed", segment ends, n, flags) or ("dense", B, N, mode), so the layouts never meet -- is offered that result as `prefix_ref` +
`prefix_in`; the kernel compares the input with it bit for bit, per cloud, before it believes the certificate.  Provenance is by
content, so nothing here has to be right for the result to be right, with two exceptions the book takes care of:

* the recorded coordinates must still be what the kernel wrote.  The book keeps a PRIVATE copy of them (3 floats per sample): the
  tensor the caller received may be written to in ways no version counter sees (`.data`, raw-pointer writes through the
  pointops_cuda shim, other kernels), and comparing a tensor with itself would always pass;
* a result is only offered on the stream that produced it (or one that ``adopt``-ed it after waiting): elsewhere nothing orders the
  reading launch after the writing one, and the caching allocator may recycle a dropped entry's memory while it is still being read.

The shortcut is OPT-IN per call site (``prefix=True``): the plain operators run every launch for real; the call sites that chain
sampling levels by construction -- the set-abstraction modules in eval mode, the Point-Transformer sampling pyramid -- ask for it.
``config.cfg.fps_prefix`` (seeded from TGN_FPS_PREFIX) forces it on (True) or off (False) everywhere; None leaves it to the call site.
"""
import torch

from . import _lib, config
from ._lib import as_int, f32c, idx32c, ops, require_cuda, stream


class PrefixBook:
    def __init__(self, cap=16):
        self.cap = cap
        self.entries = []   # (key, device, stream, private copy of the coordinates, certificate), most recent last
        self.stats = {"offered": 0}

    def clear(self):
        del self.entries[:]

    def offer(self, key, device):
        """(certificate, reference coordinates) of the most recent result with this layout, or (None, None)."""
        stream = torch.cuda.current_stream(device).cuda_stream
        for k, dev, st, ref, cert in reversed(self.entries):
            if k == key and dev == device and st == stream:
                self.stats["offered"] += 1
                return cert, ref
        return None, None

    def adopt(self, device, from_stream, to_stream):
        """`to_stream` has just been made to wait for `from_stream` (wait_stream / an event): results recorded on the latter may be
        offered on the former from now on.  The copies are marked as in use on `to_stream` for the caching allocator."""
        src, dst = from_stream.cuda_stream, to_stream.cuda_stream
        if src == dst:
            return
        have = {(k, id(ref)) for k, dev, st, ref, cert in self.entries if dev == device and st == dst}
        for k, dev, st, ref, cert in list(self.entries):
            if dev == device and st == src and (k, id(ref)) not in have:
                for t in (ref, cert):
                    if t is not None:
                        t.record_stream(to_stream)
                self.entries.append((k, dev, dst, ref, cert))
        del self.entries[:-2 * self.cap]

    def record(self, key, device, new_xyz, cert, shared):
        """Remember a result.  shared: the caller holds `new_xyz` too -- the book keeps its own copy."""
        if shared:
            new_xyz = new_xyz.detach().clone()
        self.entries.append((key, device, torch.cuda.current_stream(device).cuda_stream, new_xyz, cert))
        del self.entries[:-self.cap]


book = PrefixBook()      # at most 16 private copies of sampled coordinates, both layouts together
stats = book.stats
clear = book.clear


def adopt(from_stream, to_stream):
    """After `to_stream` has been made to wait for `from_stream`: FPS results recorded on the latter may serve the
    FPS-of-an-FPS-result shortcut on the former (the side-stream sampling pyramid of the Point-Transformer U-Net)."""
    book.adopt(from_stream.device, from_stream, to_stream)


def workspace(b, n_max, n_total, device):
    """Scratch for clouds that do not fit the register-resident FPS kernels (raw scans): the cell-sorted
    workspace of the large-cloud kernel, or -- above its 262 144-point limit -- the reference's tmp array."""
    if n_max <= ops().tgn_fps_resident_capacity():
        return None, 0
    nbytes = int(ops().tgn_fps_workspace_bytes(b, n_max))
    nbytes = max(nbytes, 4 * int(n_total))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _takes_part(site_opt_in, mode):
    """Does this call take part in the shortcut?  The switch if it is set, else the call site; never with the tree tie order."""
    forced = config.cfg.fps_prefix
    return bool(site_opt_in if forced is None else forced) and not (mode & _lib.FPS_TREE_TIES)


def _launch(entry, head, idx, new_xyz, b, n_max, n_total, flags, keys, shared, throughput=False):
    """entry(*head, ws, nbytes, idx, new_xyz, prefix_in, prefix_ref, prefix_out, flags, stream), with everything between `head` and
    `flags` made here.  keys: None when the call does not take part in the shortcut, else (what the input must look like to be
    offered a recorded result, what this result looks like)."""
    device = idx.device
    ws, nbytes = workspace(b, n_max, n_total, device)
    if throughput and nbytes == 0 and b >= 3 * torch.cuda.get_device_properties(device).multi_processor_count:
        # three or more clouds per CU: the L2-resident form shares a CU between four workgroups and finishes the BATCH sooner
        # (24 000 -> 4096: 10.9 against 12.7 us per scan at 768 scans, 9.7 at 1024; profiles/r06_fps_throughput.txt); same results
        nbytes = int(ops().tgn_fps_throughput_workspace_bytes(b, n_max))
        if nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            flags |= _lib.FPS_THROUGHPUT
    cert_in = ref = cert_out = None
    if keys:
        cert_in, ref = book.offer(keys[0], device)
        cert_out = torch.empty(b, dtype=torch.int32, device=device)
    entry(*head, ws, nbytes, idx, new_xyz, cert_in, ref, cert_out, flags, stream())
    if keys:
        book.record(keys[1], device, new_xyz, cert_out, shared=shared)


def sample_packed(xyz, offset, new_offset, cuda_compat=False, prefix=False, *, host):
    """furthestsampling that also returns the sampled coordinates xyz[idx] straight from the kernel
    (what blocks.py:69-70 computes with a second gather).  Returns (idx int32 (m,), new_xyz (m,3)).
    prefix=True: this call site chains sampling levels -- take part in the FPS-of-an-FPS-result shortcut.
    host: the values of (offset, new_offset) as lists of ints (pointops.offsets_host)."""
    require_cuda(xyz, offset, new_offset)
    xyz = f32c(xyz.detach(), "xyz")
    off_h, noff_h = host
    offset, new_offset = idx32c(offset, "offset"), idx32c(new_offset, "new_offset")
    b, n = offset.shape[0], xyz.shape[0]
    if b == 0 or noff_h[-1] == 0:      # nothing to sample (no segments, or only empty ones): an empty result, no launch
        return (torch.zeros(0, dtype=torch.int32, device=xyz.device),
                torch.zeros(0, 3, dtype=torch.float32, device=xyz.device))
    n_max, prev = 0, 0                 # the longest segment
    for end in off_h:
        n_max, prev = max(n_max, end - prev), end
    m = noff_h[-1]
    idx = torch.empty(m, dtype=torch.int32, device=xyz.device)
    new_xyz = torch.empty(m, 3, dtype=torch.float32, device=xyz.device)
    flags = _lib.fps_flags(cuda_compat)
    keys = (("packed", tuple(off_h), n, flags), ("packed", tuple(noff_h), m, flags)) if _takes_part(prefix, flags) else None
    _launch(ops().tgn_furthestsampling_prefix, (b, n_max, xyz, offset, new_offset), idx, new_xyz, b, n_max, n, flags, keys, True)
    return idx, new_xyz


def sample_dense(xyz, npoint, want_coords=False, cuda_compat=False, prefix=False, mode=None):
    """(B,N,3) -> (idx int64 (B,npoint) local to each cloud, new_xyz (B,npoint,3) or None without want_coords).
    prefix=True: this call site chains sampling levels -- every set-abstraction level after the first samples the previous level's
    new_xyz (pointnet2_utils.py:160 / :276).  mode: explicit tie-order / contraction flag bits (None: the process-wide
    _lib.set_fps_mode() setting)."""
    require_cuda(xyz)
    npoint = as_int(npoint)
    xyz = f32c(xyz.detach())
    B, N, _ = xyz.shape
    mode = _lib.fps_flags(cuda_compat) if mode is None else int(mode)
    keys = (("dense", B, N, mode), ("dense", B, npoint, mode)) if _takes_part(prefix, mode) else None
    idx = torch.empty(B, npoint, dtype=torch.int64, device=xyz.device)
    new_xyz = torch.empty(B, npoint, 3, dtype=torch.float32, device=xyz.device) if (want_coords or keys) else None   # the book's copy
    if B == 0 or npoint == 0:
        return idx, (new_xyz if want_coords else None)
    _launch(ops().tgn_furthestsampling_dense_prefix, (B, N, npoint, xyz), idx, new_xyz, B, N, B * N,
            _lib.FPS_LOCAL_INDEX | _lib.FPS_INDEX64 | mode, keys, want_coords, throughput=True)
    return idx, (new_xyz if want_coords else None)

