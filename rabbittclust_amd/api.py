"""Host-side Python mirror of the sketch + all-pairs path, over the C ABI (include/rtclust.h).

PyTorch is plumbing here: device buffers (torch tensors), the current HIP stream and
torch.distributed.  All compute goes through librtclust_hip.so; nothing in this module has a
CPU fallback.  Names follow the reference's vocabulary (genomes, sketches, hashes, MST edges).
"""
import ctypes as C
import os
import math

import numpy as np
import torch

from . import _lib
from ._lib import RtcError, SynthDesc

SYNTH_DT = np.dtype([("fam_seed", "<u8"), ("mut_seed", "<u8"), ("mut_thr", "<u4"), ("n_every", "<u4")])
CEDGE_DT = np.dtype([("i", "<u4"), ("j", "<u4"), ("common", "<u4")])
EDGE_DT = np.dtype([("preNode", "<i4"), ("sufNode", "<i4"), ("dist", "<f8")])  # edge.mst record
REP_PAIR_DT = np.dtype([("query", "<u4"), ("slot", "<u4"), ("common", "<u4"), ("pad", "<u4"), ("dist", "<f8")])  # rtc_rep_pair
REP_HIT_DT = np.dtype([("query", "<u4"), ("slot", "<u4"), ("common", "<u4"), ("denom", "<u4")])  # rtc_rep_hit
KDIST_DT = np.dtype([("common", "<u4"), ("size_p", "<u4"), ("size_q", "<u4"), ("neighbour", "<u4")])  # rtc_kdist
# Context.dbscan_sweep's curve: rtc_kdist plus the distance the host forms from it
KDIST_CURVE_DT = np.dtype(KDIST_DT.descr + [("distance", "<f8")])
KDIST_NONE = 0xFFFFFFFF  # neighbour of a point with fewer than minPts - 1 candidates (distance inf)
# rtc_dbscan_place
PLACE_DT = np.dtype([("label", "<i4"), ("label_max", "<i4"), ("n_neighbours", "<u4"), ("n_core", "<u4"), ("nearest", "<u4"),
                     ("common", "<u4"), ("denom", "<u4"), ("flags", "<u4")])
PLACE_NONE = 0xFFFFFFFF  # nearest of a query that shares no hash with the model
GEDGE_DT = np.dtype([("u", "<u4"), ("v", "<u4"), ("common", "<u4"), ("pad", "<u4")])  # rtc_gedge; pad: 0 from graph_build, the truncated denom from graph_build_mash (graph_denom reads it)
QEDGE_DT = np.dtype([("q", "<u4"), ("p", "<u4"), ("common", "<u4"), ("pad", "<u4")])  # rtc_qedge
NEAR_DT = np.dtype([("nearest", "<u4"), ("common", "<u4"), ("denom", "<u4"), ("n_candidates", "<u4"), ("n_passing", "<u4"),
                    ("n_kept", "<u4")])  # rtc_graph_near; nearest PLACE_NONE: no shared hash
PLACEMENT_DT = np.dtype([("label", "<i4"), ("runner_up", "<i4"), ("n_edges", "<u4"), ("n_comms", "<u4"), ("k_x", "<u8"), ("e_label", "<u8"),
                         ("e_runner", "<u8")])  # rtc_leiden_placement
WEDGE_DT = np.dtype([("u", "<u4"), ("v", "<u4"), ("q", "<u4")])  # rtc_wedge
LKEY_DT = np.dtype([("common", "<u4"), ("denom", "<u4")])  # rtc_lkey
LMERGE_DT = np.dtype([("a", "<u4"), ("b", "<u4"), ("common", "<u4"), ("denom", "<u4"), ("size", "<u4")])  # rtc_lmerge
NJOIN_DT = np.dtype([("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("pad", "<u4"), ("len_a", "<f8"), ("len_b", "<f8"), ("len_c", "<f8")])  # rtc_njoin
NJ_PATH_WAVE, NJ_PATH_WORKGROUP, NJ_PATH_GRID = 1, 2, 4  # rtc_nj_last_path
NJ_GRID_MIN = 256  # the library's default RTC_NJ_GRID_MIN (rtc_nj.hip: NJ_GRID_MIN)
NJ_SCAN_BLOCKS = 1024  # the default and ceiling of RTC_NJ_SCAN_BLOCKS (rtc_nj.hip: NJ_SCAN_BLOCKS)
NJ_SUPPORT_MAX = 256  # rtc_nj_support's most replicates
JK_LDS_ELEMS = 1024  # the jackknife counting kernel stages a list of up to this many hashes in LDS (csrc/rtc_jackknife.h); a longer one is searched in global memory
CSUPPORT_DT = np.dtype([("size", "<u4"), ("recovered", "<u4"), ("split", "<u4"), ("merged", "<u4"), ("mixed", "<u4"), ("max_pieces", "<u4")])  # rtc_csupport
CSUPPORT_MAX = 256  # rtc_cluster_support's most replicates (csrc/rtc_support.h: CSUP_MAX_REPLICATES)
CSUPPORT_TABLE_MAX = 1 << 25  # the keep table's most entries (csrc/rtc_support.h: CSUP_TABLE_MAX)
UMERGE_DT = np.dtype([("a", "<u4"), ("b", "<u4"), ("size_a", "<u4"), ("size_b", "<u4"), ("sum", "<u8")])  # rtc_umerge
UPGMA_PATH_WAVE, UPGMA_PATH_WORKGROUP, UPGMA_PATH_GRID = 1, 2, 4  # rtc_upgma_last_path
UPGMA_GRID_MIN = 128  # the library's default RTC_UPGMA_GRID_MIN (rtc_upgma.h: UPGMA_GRID_MIN)
UPGMA_SCAN_BLOCKS = 1024  # the default and ceiling of RTC_UPGMA_SCAN_BLOCKS (rtc_upgma.h: UPGMA_SCAN_BLOCKS)
UPGMA_Q1 = 1 << 20  # distance 1 in the units of rtc_upgma_dev's sums
HEDGE_DT = np.dtype([("p", "<u4"), ("q", "<u4"), ("common", "<u4"), ("size_p", "<u4"), ("size_q", "<u4")])  # rtc_hedge
MCL_ENTRY_DT = np.dtype([("col", "<u4"), ("row", "<u4"), ("value", "<u4"), ("pad", "<u4")])  # rtc_mcl_entry
MCL_PATH_WAVE, MCL_PATH_WORKGROUP, MCL_PATH_GLOBAL = 1, 2, 4  # rtc_mcl_last_path
# the column kernel's path boundaries (csrc/rtc_mcl.h): a column whose expansion gathers at most MCL_WAVE_WORK products takes one
# wave, at most MCL_BLOCK_WORK a 256-lane workgroup, more the table in global memory
MCL_WAVE_WORK = 256
MCL_BLOCK_WORK = 3072
SNN_DT = np.dtype([("shared", "<u4"), ("deg_u", "<u4"), ("deg_v", "<u4"), ("flags", "<u4")])  # rtc_snn
SNN_PATH_WAVE, SNN_PATH_WORKGROUP, SNN_PATH_GLOBAL = 1, 2, 4  # rtc_graph_snn_last_path
# the counting kernel's path boundaries (csrc/rtc_snn.h): a record whose longer row has at most SNN_WAVE_ROW entries takes one
# wave, at most SNN_BLOCK_ROW a 256-lane workgroup, both with that row in LDS; a longer one is searched in global memory
SNN_WAVE_ROW = 768
SNN_BLOCK_ROW = 8192
DEGREE_PLACE_DT = np.dtype([("rep", "<u4"), ("degree", "<u4"), ("common", "<u4"), ("denom", "<u4")])  # rtc_degree_place
DEGREE_PATH_WAVE, DEGREE_PATH_WORKGROUP, DEGREE_PATH_TAIL = 1, 2, 4  # rtc_greedy_degree_last_path
DEGREE_WAVE_ROW = 4096  # a member with more candidate representatives takes the 256-lane path (csrc/rtc_topk_select.h: TK_LONG)
SIL_DT = np.dtype([("a_num", "<u8"), ("b_num", "<u8"), ("a_den", "<u4"), ("b_den", "<u4"), ("b_cluster", "<u4"), ("far_q", "<u4"),
                   ("near_q", "<u4"), ("near_cluster", "<u4")])  # rtc_sil
SIL_ONE = 1 << 20  # distance 1 in rtc_silhouette's units
SIL_NONE = 0xFFFFFFFF  # b_cluster / near_cluster: none
SIL_PATH_WAVE, SIL_PATH_WORKGROUP, SIL_PATH_GLOBAL = 1, 2, 4  # rtc_silhouette_last_path
# the row kernel's path boundaries (csrc/rtc_quality.h): a row of at most SIL_WAVE_ROW entries takes one wave and a table of
# SIL_WAVE_SLOTS slots in LDS, one of at most SIL_BLOCK_ROW a 256-lane workgroup and SIL_BLOCK_SLOTS slots, a longer one a table of
# 1 << max(SIL_GLOBAL_LOG2_MIN, ceil(log2(2 entries))) slots in global memory
SIL_WAVE_ROW, SIL_WAVE_SLOTS = 128, 256
SIL_BLOCK_ROW, SIL_BLOCK_SLOTS = 1024, 2048
SIL_GLOBAL_LOG2_MIN = 6
SCREEN_HIT_DT = np.dtype([("query", "<u4"), ("slot", "<u4"), ("common", "<u4"), ("size", "<u4"), ("unique", "<u4"), ("rank", "<u4")])  # rtc_screen_hit
SCREEN_SUM_DT = np.dtype([("n_hashes", "<u4"), ("n_matched", "<u4"), ("n_explained", "<u4"), ("n_hits", "<u4"), ("n_picks", "<u4"),
                          ("pad", "<u4")])  # rtc_screen_sum
SCREEN_PATH_WAVE, SCREEN_PATH_BLOCK, SCREEN_PATH_GLOBAL = 1, 2, 4  # rtc_rep_screen_last_path
# the gather kernel's path boundaries (csrc/rtc_screen.h): a sample with at most SCREEN_WAVE_CANDS eligible candidates takes one
# wave, one with at most SCREEN_BLOCK_CANDS a 256-lane workgroup, both with the remaining counts in LDS; more: the counts in global
# memory.  SCREEN_POS_BYTES a sample hash and SCREEN_MATCH_BYTES a match record are what a chunk is charged against RTC_SCREEN_BYTES.
SCREEN_WAVE_CANDS = 512
SCREEN_BLOCK_CANDS = 4096
SCREEN_POS_BYTES = 40
SCREEN_MATCH_BYTES = 72
SCREEN_Q20 = 1 << 20  # containment 1 in rtc_rep_screen's min_cont_q20
PAN_DT = np.dtype([("total", "<u8"), ("pan", "<u8"), ("core", "<u8"), ("soft", "<u8"), ("shell", "<u8"), ("cloud", "<u8"), ("single", "<u8"),
                   ("size", "<u4"), ("pad", "<u4")])  # rtc_pan
PAN_GENOME_DT = np.dtype([("occ_sum", "<u8"), ("unique", "<u4"), ("core", "<u4"), ("soft", "<u4"), ("shell", "<u4"), ("cloud", "<u4"),
                          ("pad", "<u4")])  # rtc_pan_genome
PAN_PATH_WAVE, PAN_PATH_BLOCK, PAN_PATH_GLOBAL = 1, 2, 4  # rtc_pangenome_last_path
# the cluster paths' boundaries (csrc/rtc_pan.h): a cluster of at most PAN_WAVE_RECORDS records (the sum of its members' sketch
# lengths) takes one wave with a table of PAN_WAVE_SLOTS slots and a histogram of PAN_WAVE_HIST entries in LDS, one of at most
# PAN_BLOCK_RECORDS a 256-lane workgroup likewise, a larger one a table of 1 << max(PAN_GLOBAL_LOG2_MIN, ceil(log2(2 records)))
# slots in the arena in global memory.  PAN_SLOT_BYTES a slot, PAN_MEMBER_BYTES a member and PAN_CLUSTER_BYTES a cluster are what
# a group of clusters is charged against RTC_PAN_BYTES.
PAN_WAVE_RECORDS, PAN_WAVE_SLOTS, PAN_WAVE_HIST = 512, 1024, 512
PAN_BLOCK_RECORDS, PAN_BLOCK_SLOTS, PAN_BLOCK_HIST = 2048, 4096, 1024
PAN_GLOBAL_LOG2_MIN = 8
PAN_GLOBAL_WGS_PER_CU = 16  # the arena's count and look-up kernels take a member a wave: 4 * PAN_GLOBAL_WGS_PER_CU waves a CU a turn
PAN_WAVE_WGS_PER_CU, PAN_BLOCK_WGS_PER_CU = 11, 3  # the LDS paths' grids: at most so many workgroups a CU, a cluster a workgroup and turn
PAN_SWEEP_BINS = 1024  # the arena's sweep keeps the counts 2 .. PAN_SWEEP_BINS + 1 in bins in LDS; larger ones go to the histogram one by one
PAN_SLOT_BYTES, PAN_MEMBER_BYTES, PAN_CLUSTER_BYTES = 12, 56, 48
PAN_EMPTY = 0xFFFFFFFFFFFFFFFF  # the empty slot's key; a hash of this value is counted beside the table
PAN_MULT = 0x9E3779B97F4A7C15
PAN_GROWTH_POINTS = 256


def pan_slot(hash_value, log2_slots):
    """The slot a hash's probe starts from in a table of 1 << log2_slots slots (csrc/rtc_pangenome.hip: pan_slot); the probe
    goes on to the next slot, wrapping."""
    return ((int(hash_value) * PAN_MULT) & 0xFFFFFFFFFFFFFFFF) >> (64 - int(log2_slots))


def pan_table_log2(records, all_global=False):
    """log2 of the slots of the arena table of a cluster of `records` records, or None for a cluster on an LDS path."""
    if not all_global and records <= PAN_BLOCK_RECORDS:
        return None
    lg = PAN_GLOBAL_LOG2_MIN
    while (1 << lg) < 2 * records:
        lg += 1
    return lg


def pan_cluster_bytes(records, members, all_global=False):
    """What rtc_pangenome charges a cluster of `members` members and `records` records against RTC_PAN_BYTES."""
    lg = pan_table_log2(records, all_global)
    return PAN_SLOT_BYTES * ((1 << lg) if lg is not None else 0) + PAN_MEMBER_BYTES * members + PAN_CLUSTER_BYTES


def pan_growth(hist, threads=1):
    """rtc_pan_growth: (j, pan, core) -- the expected pangenome and core size after j of the m = len(hist) members of a cluster
    whose histogram is hist (entry f - 1: the hashes held by f members), over all orders of the members, at j = 1 .. m or, past
    256 members, at 256 values of j from 1 to m."""
    h = np.ascontiguousarray(np.asarray(hist, dtype=np.uint64).reshape(-1))
    m = len(h)
    P = min(m, PAN_GROWTH_POINTS)
    j = np.zeros(max(P, 1), dtype=np.uint32)
    pan = np.zeros(max(P, 1), dtype=np.float64)
    core = np.zeros(max(P, 1), dtype=np.float64)
    got = C.c_uint32(0)
    st = _lib.load().rtc_pan_growth(_np_ptr(h), m, int(threads), _np_ptr(j), _np_ptr(pan), _np_ptr(core), C.byref(got))
    if st != _lib.RTC_OK:
        raise RtcError(st, "rtc_pan_growth")
    return j[:got.value].copy(), pan[:got.value].copy(), core[:got.value].copy()


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _t_ptr(t):
    return C.c_void_p(t.data_ptr())


class SketchSet:
    """Device-resident sketches: `hashes` flat tensor (int64 view of u64, or int32 view of u32),
    `start` (int64, element offsets) and `len` (int32) per genome -- the CSR the pair kernels read."""

    def __init__(self, hashes, start, length, width, k, kind):
        self.hashes, self.start, self.len, self.width, self.k, self.kind = hashes, start, length, width, k, kind

    @property
    def n(self):
        return int(self.len.numel())

    def to_host(self):
        np_dt = np.uint64 if self.width == 8 else np.uint32
        flat = self.hashes.cpu().numpy().view(np_dt).reshape(-1)
        start = self.start.cpu().numpy().astype(np.uint64)
        ln = self.len.cpu().numpy().astype(np.uint32)
        return [flat[int(s):int(s) + int(l)].copy() for s, l in zip(start, ln)]

    @staticmethod
    def from_host(sketches, device, k=21, kind="minhash", width=8):
        np_dt = np.uint64 if width == 8 else np.uint32
        t_dt = torch.int64 if width == 8 else torch.int32
        lens = np.array([len(s) for s in sketches], dtype=np.int32)
        start = np.zeros(len(sketches), dtype=np.int64)
        if len(sketches) > 1:
            start[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        flat = (np.concatenate([np.asarray(s, dtype=np_dt) for s in sketches])
                if len(sketches) and lens.sum() else np.zeros(0, dtype=np_dt))
        flat = np.ascontiguousarray(flat)
        h = torch.from_numpy(flat.view(np.int64 if width == 8 else np.int32).copy()).to(device)
        if h.numel() == 0:
            h = torch.zeros(2, dtype=t_dt, device=device)
        return SketchSet(h, torch.from_numpy(start).to(device), torch.from_numpy(lens).to(device), width, k, kind)


_LIVE = None  # weak set of the live contexts (reload_all_options)


def reload_all_options():
    """every live Context reads the RTC_* switches again (the library reads them once, at rtc_ctx_create): tests that flip one"""
    for c in list(_LIVE or ()):
        if c.h:
            c.reload_options()


class Context:
    """One context per GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RtcError(_lib.RTC_ERR_HIP, "no HIP device visible: the MI355X path has no CPU fallback")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        torch.cuda.init()
        torch.empty(1, device=self.device)  # force the HIP runtime torch bundles to initialise first
        h = C.c_void_p()
        st = self.lib.rtc_ctx_create(device, C.byref(h))
        if st != _lib.RTC_OK:
            raise RtcError(st, "rtc_ctx_create: " + self.lib.rtc_last_error(None).decode(errors="replace"))
        self.h = h
        global _LIVE
        if _LIVE is None:
            import weakref
            _LIVE = weakref.WeakSet()
        _LIVE.add(self)
        self.use_torch_stream()

    def close(self):
        if getattr(self, "h", None):
            self.lib.rtc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st):
        if st != _lib.RTC_OK:
            raise RtcError(st, self.lib.rtc_last_error(self.h).decode(errors="replace"))

    def reload_options(self):
        """the library's RTC_* switches are read when the context is created: read them again (tests that flip one)"""
        self.check(self.lib.rtc_ctx_reload_options(self.h))

    def env(self, **switches):
        """context manager: RTC_* switches set in the environment (None: unset) and read by this context, restored on exit"""
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = {k: os.environ.get(k) for k in switches}
            try:
                for k, v in switches.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = str(v)
                self.reload_options()
                yield self
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
                self.reload_options()
        return scope()

    def num_cu(self):
        info = (C.c_int * 3)()
        self.check(self.lib.rtc_device_info(self.h, info))
        return int(info[0])

    def use_torch_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.check(self.lib.rtc_ctx_set_stream(self.h, C.c_void_p(s)))

    def sync(self):
        self.check(self.lib.rtc_ctx_sync(self.h))

    def pair_last_path(self):
        """Path of the last pair_edges call: 0 none, 1 merge kernel, 2 tiled kernel, 3 inverted join."""
        return int(self.lib.rtc_pair_last_path(self.h))

    def diag(self):
        """rtc_diag_counters as a dict: which paths this context has taken since it was created"""
        a = (C.c_uint64 * 8)()
        self.check(self.lib.rtc_diag_counters(self.h, a))
        names = ("join_tiles", "tiled_tiles", "merge_tiles", "contractions", "greedy_global", "greedy_blocks", "estimates",
                 "repmatch_chunks")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def pair_last_kernel_ms(self):
        """Duration of the last tiled pair kernel launch (HIP events on its launch stream)."""
        ms = C.c_float()
        self.check(self.lib.rtc_pair_last_kernel_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def timer_start(self):
        self.check(self.lib.rtc_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self.check(self.lib.rtc_timer_stop(self.h, C.byref(ms)))
        return float(ms.value)

    # ---- inputs -------------------------------------------------------------------------------
    def synth_genomes(self, desc, off):
        """desc: numpy SYNTH_DT[n]; off: u64[n+1].  Returns uint8 tensor with all genomes."""
        desc = np.ascontiguousarray(desc, dtype=SYNTH_DT)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(desc)
        seq = torch.empty(int(off[-1]) + 64, dtype=torch.uint8, device=self.device)
        self.check(self.lib.rtc_synth_genomes_dev(self.h, _np_ptr(desc), _np_ptr(off), n, _t_ptr(seq)))
        return seq

    def upload_sequences(self, seq_np):
        t = torch.empty(len(seq_np) + 64, dtype=torch.uint8, device=self.device)
        t[:len(seq_np)] = torch.from_numpy(np.array(seq_np, dtype=np.uint8, copy=True)).to(self.device)
        return t

    # ---- sketching ----------------------------------------------------------------------------
    def sketch_minhash(self, seq, off, k=21, size=1000, sizes=None, seed=42):
        """Sketch::MinHash(k,size) + update() + storeMinHashes() for every genome.
        Returns a SketchSet (strided: start[g] = g*stride)."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
            stride = int(sizes.max()) if n else 1
        else:
            stride = int(size)
        stride = max(stride, 1)
        out = torch.empty((max(n, 1), stride), dtype=torch.int64, device=self.device)
        cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        self.check(self.lib.rtc_sketch_minhash_dev(
            self.h, _t_ptr(seq), _np_ptr(off), n, k, seed,
            _np_ptr(sizes) if sizes is not None else None, int(size), _t_ptr(out), stride, _t_ptr(cnt)))
        start = torch.arange(n, dtype=torch.int64, device=self.device) * stride
        return SketchSet(out.view(-1), start, cnt[:n], 8, k, "minhash")

    def sketch_minhash_plan(self, k=21, size=1000):
        """What the MinHash sketch calls plan for a largest sketch size `size`: dict(wgs_per_cu, packed_tables, lds_bytes)."""
        wgs, pk, lds = C.c_int(0), C.c_int(0), C.c_uint64(0)
        self.check(self.lib.rtc_sketch_minhash_plan(self.h, int(k), int(size), C.byref(wgs), C.byref(pk), C.byref(lds)))
        return {"wgs_per_cu": wgs.value, "packed_tables": bool(pk.value), "lds_bytes": lds.value}

    def sketch_minhash_into(self, seq, off, out, cnt, k=21, size=1000, sizes=None, seed=42):
        """Same as sketch_minhash, into caller-provided rows: `out` (len(off)-1, stride) int64 and `cnt`
        int32 views (used by the multi-GPU step, which sketches in two parts so that the all-gather
        of the first overlaps the sketching of the second).  `off` may start at any base offset."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        assert out.is_contiguous() and cnt.is_contiguous() and out.shape[0] == n and cnt.shape[0] == n
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        self.check(self.lib.rtc_sketch_minhash_dev(
            self.h, _t_ptr(seq), _np_ptr(off), n, k, seed,
            _np_ptr(sizes) if sizes is not None else None, int(size), _t_ptr(out), int(out.shape[1]), _t_ptr(cnt)))

    def sketch_minhash_packed(self, packed, off, k=21, size=1000, sizes=None, seed=42, n_bases=None, runs=None, out=None, cnt=None):
        """sketch_minhash over a batch in the 2-bit staging format (a PackedBatch, or `packed` uint8 device tensor of
        n_bases / 4 bytes with `runs` int64 (start, length) pairs).  `out` / `cnt`: caller-provided rows as in sketch_minhash_into."""
        if isinstance(packed, PackedBatch):
            packed, n_bases, runs = packed.packed, packed.n_bases, packed.runs
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
            stride = int(sizes.max()) if n else 1
        else:
            stride = int(size)
        stride = max(stride, 1)
        if out is None:
            out = torch.empty((max(n, 1), stride), dtype=torch.int64, device=self.device)
            cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        else:
            assert out.is_contiguous() and cnt.is_contiguous() and out.shape[0] >= n and cnt.shape[0] >= n
            stride = int(out.shape[1])
        n_runs = int(runs.numel() // 2) if runs is not None else 0
        self.check(self.lib.rtc_sketch_minhash_packed_dev(
            self.h, _t_ptr(packed), int(n_bases), _t_ptr(runs) if n_runs else None, n_runs, _np_ptr(off), n, k, seed,
            _np_ptr(sizes) if sizes is not None else None, int(size), _t_ptr(out), stride, _t_ptr(cnt)))
        start = torch.arange(n, dtype=torch.int64, device=self.device) * stride
        return SketchSet(out.view(-1), start, cnt[:n], 8, k, "minhash")

    def sketch_kssd(self, seq, off, shuffled_dim, kmer_size=21, drlevel=3, stride=None):
        """sketchFileWithKssd's per-file body.  shuffled_dim: int32[2^(4*half_subk)] from the host."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        sd = np.ascontiguousarray(shuffled_dim, dtype=np.int32)
        half_k = (kmer_size + 1) // 2
        use64 = half_k - drlevel > 8
        maxlen = int((off[1:] - off[:-1]).max()) if n else 0
        if stride is None:
            keep = 1.0 / (16 ** drlevel)
            stride = int(maxlen * keep * 1.5) + 256
        while True:
            t_dt = torch.int64 if use64 else torch.int32
            out = torch.empty((max(n, 1), stride), dtype=t_dt, device=self.device)
            cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
            width = C.c_int()
            need = C.c_uint32()
            st = self.lib.rtc_sketch_kssd_dev(self.h, _t_ptr(seq), _np_ptr(off), n, kmer_size, drlevel,
                                              _np_ptr(sd), _t_ptr(out), stride, _t_ptr(cnt),
                                              C.byref(width), C.byref(need))
            if st == _lib.RTC_ERR_OVERFLOW:
                stride = int(need.value) + 64
                continue
            self.check(st)
            break
        start = torch.arange(n, dtype=torch.int64, device=self.device) * stride
        return SketchSet(out.view(-1), start, cnt[:n], int(width.value), half_k * 2, "kssd")

    def sketch_kssd_packed(self, packed, n_bases, runs, off, shuffled_dim, kmer_size=21, drlevel=3, stride=None):
        """sketch_kssd over a batch in the 2-bit staging format: `packed` uint8 device tensor of n_bases / 4 bytes,
        `runs` int64 device tensor of (start, length) pairs (ascending, disjoint) for everything outside ACGT.
        (`packed` may be a PackedBatch; n_bases and runs are then taken from it.)"""
        if isinstance(packed, PackedBatch):
            packed, n_bases, runs = packed.packed, packed.n_bases, packed.runs
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        sd = np.ascontiguousarray(shuffled_dim, dtype=np.int32)
        half_k = (kmer_size + 1) // 2
        use64 = half_k - drlevel > 8
        maxlen = int((off[1:] - off[:-1]).max()) if n else 0
        if stride is None:
            stride = int(maxlen / (16 ** drlevel) * 1.5) + 256
        n_runs = int(runs.numel() // 2) if runs is not None else 0
        while True:
            out = torch.empty((max(n, 1), stride), dtype=torch.int64 if use64 else torch.int32, device=self.device)
            cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
            width = C.c_int()
            need = C.c_uint32()
            st = self.lib.rtc_sketch_kssd_packed_dev(self.h, _t_ptr(packed), int(n_bases), _t_ptr(runs) if n_runs else None,
                                                     n_runs, _np_ptr(off), n, kmer_size, drlevel, _np_ptr(sd), _t_ptr(out),
                                                     stride, _t_ptr(cnt), C.byref(width), C.byref(need))
            if st == _lib.RTC_ERR_OVERFLOW:
                stride = int(need.value) + 64
                continue
            self.check(st)
            break
        start = torch.arange(n, dtype=torch.int64, device=self.device) * stride
        return SketchSet(out.view(-1), start, cnt[:n], int(width.value), half_k * 2, "kssd")

    # ---- all pairs ----------------------------------------------------------------------------
    def pair_common(self, sk, row0=0, row1=None, col0=0, col1=None, lower_only=False, algo=0, out=None):
        n = sk.n
        row1 = n if row1 is None else row1
        col1 = n if col1 is None else col1
        ld = col1 - col0
        if out is None:
            out = torch.zeros((max(row1 - row0, 1), max(ld, 1)), dtype=torch.int32, device=self.device)
        self.check(self.lib.rtc_pair_common_dev(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start),
                                                _t_ptr(sk.len), n, row0, row1, col0, col1, _t_ptr(out),
                                                out.stride(0), int(lower_only), algo))
        return out

    def pair_mash(self, sk, sketch_size, row0=0, row1=None, col0=0, col1=None):
        """Mash's union-truncated estimator per pair (modifyMST's distance(), D3): (common, denom) tensors."""
        n = sk.n
        row1 = n if row1 is None else row1
        col1 = n if col1 is None else col1
        shape = (max(row1 - row0, 1), max(col1 - col0, 1))
        common = torch.zeros(shape, dtype=torch.int32, device=self.device)
        denom = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.check(self.lib.rtc_pair_mash_dev(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n,
                                              int(sketch_size), row0, row1, col0, col1, _t_ptr(common), _t_ptr(denom),
                                              common.stride(0)))
        return common, denom

    def pair_mash_edges(self, sk, sketch_size, pairs):
        """rtc_pair_mash_edges_dev: pair_mash's (common, denom) for the given pairs alone, an (m, 2) array of indices below sk.n,
        by the recount kernel of dbscan_mash.  Returns two uint32 arrays of m entries."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        m = len(pairs)
        if m and (pairs.min() < 0 or pairs.max() >= sk.n):
            raise ValueError("pair_mash_edges: an index outside [0, n)")
        edges = np.zeros(max(m, 1), dtype=CEDGE_DT)
        edges["i"][:m], edges["j"][:m] = pairs[:, 0], pairs[:, 1]
        d_edges = torch.from_numpy(edges.view(np.uint32).reshape(-1, 3).view(np.int32)).to(self.device)
        common = torch.zeros(max(m, 1), dtype=torch.int32, device=self.device)
        denom = torch.zeros(max(m, 1), dtype=torch.int32, device=self.device)
        self.check(self.lib.rtc_pair_mash_edges_dev(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), sk.n,
                                                    int(sketch_size), _t_ptr(d_edges), m, _t_ptr(common), _t_ptr(denom)))
        self.sync()
        return common[:m].cpu().numpy().view(np.uint32), denom[:m].cpu().numpy().view(np.uint32)

    def extract_edges(self, common, sk, row0, row1, col0, col1, radio, cap):
        edges = torch.empty((max(cap, 1), 3), dtype=torch.int32, device=self.device)
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.check(self.lib.rtc_extract_edges_dev(self.h, _t_ptr(common), common.stride(0), row0, row1,
                                                  col0, col1, _t_ptr(sk.len), radio, _t_ptr(edges), cap,
                                                  _t_ptr(count)))
        return edges, count

    def mst_dense(self, sk, threshold, is_containment=False, span=100, start_index=0):
        """rtc_mst_dense: (edge.mst records, dense[span, n] int32, ani[101] u64) -- the --dense by-products."""
        n = sk.n
        out = np.zeros(max(n, 1), dtype=EDGE_DT)
        dense = np.zeros((span, max(n, 1)), dtype=np.int32)
        ani = np.zeros(101, dtype=np.uint64)
        m = C.c_uint64()
        self.check(self.lib.rtc_mst_dense(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n,
                                          int(start_index), sk.k, int(is_containment), float(threshold), _np_ptr(out),
                                          C.byref(m), span, _np_ptr(dense), _np_ptr(ani)))
        return out[:m.value].copy(), dense[:, :n], ani

    def pair_edges(self, sk, row0, row1, col0, col1, radio, cap):
        """Fused form of pair_common + extract_edges (no dense matrix).  Returns (edges, count)."""
        edges = torch.empty((max(cap, 1), 3), dtype=torch.int32, device=self.device)
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.check(self.lib.rtc_pair_edges_dev(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len),
                                               sk.n, row0, row1, col0, col1, int(radio), _t_ptr(edges), cap,
                                               _t_ptr(count)))
        return edges, int(count.item())

    def msf(self, edges, lens, wmode=0):
        """rtc_msf_dev: the minimum spanning forest of a candidate list.  edges: (i, j, common) rows, a host array or a device
        tensor [m, 3] int32; lens: the sizes, one per vertex.  Returns (the forest's CEDGE_DT records in (weight key, i, j)
        order, the Boruvka rounds the call ran)."""
        def dev(a):
            if not torch.is_tensor(a):
                a = np.ascontiguousarray(a)
                a = torch.from_numpy((a if a.dtype.itemsize == 4 else a.astype(np.uint32)).view(np.int32).copy())
            return a.to(self.device).contiguous()
        edges, lens = dev(edges).reshape(-1, 3), dev(lens).reshape(-1)
        n, m = int(lens.numel()), int(edges.shape[0])
        sel = torch.empty((max(n, 1), 3), dtype=torch.int32, device=self.device)
        nsel, rounds = C.c_uint64(), C.c_int()
        self.check(self.lib.rtc_msf_dev(self.h, _t_ptr(edges) if m else None, m, _t_ptr(lens), n, int(wmode), _t_ptr(sel),
                                        C.byref(nsel), C.byref(rounds)))
        rec = np.ascontiguousarray(sel[:nsel.value].cpu().numpy().view(np.uint32)).view(CEDGE_DT).reshape(-1)
        return rec, int(rounds.value)

    def mst(self, sk, threshold, is_containment=False, start_index=0):
        """compute_minhash_mst / compute_kssd_mst: returns numpy EDGE_DT array (edge.mst records).
        start_index > 0: only rows >= start_index (the --append form, src/MST.cpp:1375-1383)."""
        n = sk.n
        out = np.zeros(max(n, 1), dtype=EDGE_DT)
        m = C.c_uint64()
        self.check(self.lib.rtc_mst_append(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len),
                                           n, int(start_index), sk.k, int(is_containment), float(threshold),
                                           _np_ptr(out), C.byref(m)))
        return out[:m.value].copy()

    def sketch_minhash_sharded(self, comm, seq, off, k=21, size=1000, sizes=None, stride=None, seed=42):
        """Multi-GPU sketch phase behind the C ABI: this rank's genomes into its block of the canonical
        global buffers, gathered to every rank (two parts, the first gather overlapping the second
        sketch launch).  Returns the global SketchSet (comm.size * n_local genomes)."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n_local = len(off) - 1
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        if stride is None:
            stride = int(sizes.max()) if sizes is not None else int(size)
            if sizes is not None and comm.size > 1:  # per-rank maxima differ: agree
                stride = int(comm.all_reduce_host([stride], "max")[0])
        n = comm.size * n_local
        out = torch.empty((max(n, 1), max(stride, 1)), dtype=torch.int64, device=self.device)
        cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        self.check(self.lib.rtc_sketch_minhash_sharded(
            self.h, comm.h, _t_ptr(seq), _np_ptr(off), n_local, k, seed,
            _np_ptr(sizes) if sizes is not None else None, int(size), _t_ptr(out), max(stride, 1), _t_ptr(cnt)))
        start = torch.arange(n, dtype=torch.int64, device=self.device) * max(stride, 1)
        return SketchSet(out.view(-1), start, cnt[:n], 8, k, "minhash")

    def sketch_packed_sharded(self, comm, batches, mode="minhash", k=21, size=1000, seed=42, drlevel=3, shuffled_dim=None,
                              stride=None, out=None, cnt=None):
        """Multi-GPU sketch phase behind the C ABI for a rank whose genomes are resident as batches in the 2-bit staging
        format: `batches` = [(PackedBatch, off), ...] in the order of the rank's rows (every rank: the same batch sizes).
        rtc_sketch_minhash_packed_sharded / rtc_sketch_kssd_packed_sharded per batch; a batch's gather travels beside the
        next batch's sketch kernel.  Returns the global SketchSet (comm.size * n_local genomes, canonical order).
        `out` / `cnt`: caller-provided global rows (reused between steps)."""
        offs = [np.ascontiguousarray(o, dtype=np.uint64) for _, o in batches]
        n_local = sum(len(o) - 1 for o in offs)
        n = comm.size * n_local
        kssd = mode == "kssd"
        if kssd:
            sd = np.ascontiguousarray(shuffled_dim, dtype=np.int32)
            half_k = (k + 1) // 2
            width = 8 if half_k - drlevel > 8 else 4
            kk = half_k * 2
            if stride is None:  # 1.25 x the expected count of the longest genome: ample for genomes of one length
                longest = max(int((o[1:] - o[:-1]).max()) for o in offs)
                stride = (int(longest / (16 ** drlevel) * 1.25) + 64 + 3) // 4 * 4
                stride = int(comm.all_reduce_host([stride], "max")[0])
        else:
            width, kk = 8, k
            stride = int(size) if stride is None else int(stride)
        t_dt = torch.int64 if width == 8 else torch.int32
        while True:
            if out is None or out.shape != (max(n, 1), stride) or out.dtype != t_dt:
                out = torch.empty((max(n, 1), stride), dtype=t_dt, device=self.device)
                cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
            row = 0
            st = _lib.RTC_OK
            need = C.c_uint32()
            for i, ((pb, _), off) in enumerate(zip(batches, offs)):
                nb = len(off) - 1
                last = int(i == len(batches) - 1)
                n_runs = int(pb.runs.numel() // 2) if pb.runs is not None else 0
                runs = _t_ptr(pb.runs) if n_runs else None
                if kssd:
                    w = C.c_int()
                    st = self.lib.rtc_sketch_kssd_packed_sharded(self.h, comm.h, _t_ptr(pb.packed), pb.n_bases, runs, n_runs, _np_ptr(off), nb,
                                                                 row, n_local, last, k, drlevel, _np_ptr(sd), _t_ptr(out), stride,
                                                                 _t_ptr(cnt), C.byref(w), C.byref(need))
                else:
                    st = self.lib.rtc_sketch_minhash_packed_sharded(self.h, comm.h, _t_ptr(pb.packed), pb.n_bases, runs, n_runs, _np_ptr(off),
                                                                    nb, row, n_local, last, k, seed, None, int(size), _t_ptr(out), stride,
                                                                    _t_ptr(cnt))
                if st != _lib.RTC_OK:
                    break
                row += nb
            if kssd and st == _lib.RTC_ERR_OVERFLOW:  # every rank got it, with the same need: wider rows, once more
                stride = (int(need.value) + 64 + 3) // 4 * 4
                out = None
                continue
            self.check(st)
            break
        start = torch.arange(n, dtype=torch.int64, device=self.device) * stride
        return SketchSet(out.view(-1), start, cnt[:n], width, kk, "kssd" if kssd else "minhash")

    def mst_sharded(self, comm, sk, threshold, is_containment=False):
        """rtc_mst across the ranks of `comm`; returns (edge.mst records, ShardStats)."""
        n = sk.n
        out = np.empty(max(n, 1), dtype=EDGE_DT)  # (the call writes the first m records; the caller gets a view of them)
        m = C.c_uint64()
        stats = _lib.ShardStats()
        self.check(self.lib.rtc_mst_sharded(self.h, comm.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len),
                                            n, sk.k, int(is_containment), float(threshold), _np_ptr(out), C.byref(m),
                                            C.byref(stats)))
        return out[:m.value], stats

    def mst_mash(self, sk, sketch_size, is_containment=False, start_index=0, span=0):
        """modifyMST (the dense loop): spanning tree over EVERY pair, Mash-estimator / containDistance weights.
        Returns edge.mst records {i < j}; with span > 0 also (dense[span, n], ani[101])."""
        n = sk.n
        out = np.zeros(max(n, 1), dtype=EDGE_DT)
        dense = np.zeros((max(span, 1), max(n, 1)), dtype=np.int32)
        ani = np.zeros(101, dtype=np.uint64)
        m = C.c_uint64()
        self.check(self.lib.rtc_mst_mash(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n,
                                         int(start_index), sk.k, int(is_containment), int(sketch_size), _np_ptr(out),
                                         C.byref(m), int(span), _np_ptr(dense) if span else None, _np_ptr(ani) if span else None))
        return (out[:m.value].copy(), dense[:, :n], ani) if span else out[:m.value].copy()

    def greedy_mash(self, sk, threshold, sketch_size, is_containment=False):
        """greedyCluster (legacy loop, every representative, Mash estimator): (n_clusters, rep_of)."""
        n = sk.n
        rep = np.zeros(max(n, 1), dtype=np.int32)
        nc = C.c_uint32()
        self.check(self.lib.rtc_greedy_mash(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, sk.k,
                                            int(is_containment), int(sketch_size), float(threshold), _np_ptr(rep), C.byref(nc)))
        return int(nc.value), rep[:n].copy()

    def greedy(self, sk, threshold, size_cfg=None, is_containment=False):
        n = sk.n
        rep = np.zeros(max(n, 1), dtype=np.int32)
        nc = C.c_uint32()
        cfg = None
        if size_cfg is not None:
            cfg = np.ascontiguousarray(np.broadcast_to(np.asarray(size_cfg, dtype=np.uint32), (n,)))
        self.check(self.lib.rtc_greedy(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len),
                                       n, _np_ptr(cfg) if cfg is not None else None, sk.k,
                                       int(is_containment), int(sk.kind == "kssd"), float(threshold),
                                       _np_ptr(rep), C.byref(nc)))
        return int(nc.value), rep[:n].copy()

    def greedy_degree(self, sk, threshold, kmer_size, sketch_size=None):
        """clust-greedy --order degree (rtc_greedy_degree): the clusters include/rtclust.h defines over the neighbour graph at
        `threshold` -- KSSD sketches with sketch_size None (rtc_dbscan's predicate), MinHash sketches of at most sketch_size
        hashes otherwise (rtc_mash_distance <= threshold).  Returns (rep, degree, common, denom, n_clusters): uint32 arrays
        with one entry per genome, rep[v] == v for a representative, common / denom those of the pair (v, rep[v])."""
        n = sk.n
        out = np.zeros(max(n, 1), dtype=DEGREE_PLACE_DT)
        nc = C.c_uint32()
        self.check(self.lib.rtc_greedy_degree(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n,
                                              int(sketch_size is not None), int(sketch_size or 0), float(threshold), int(kmer_size),
                                              _np_ptr(out), C.byref(nc)))
        out = out[:n]
        return out["rep"].copy(), out["degree"].copy(), out["common"].copy(), out["denom"].copy(), int(nc.value)

    def greedy_degree_counters(self):
        """rtc_greedy_degree_counters as a dict (the last greedy_degree call), the two packed words taken apart."""
        a = (C.c_uint64 * 12)()
        self.check(self.lib.rtc_greedy_degree_counters(self.h, a))
        names = ("chunks", "candidate_edges", "merged", "kept_edges", "representatives", None, None, "pair_ns", "predicate_ns",
                 "select_ns", "assign_ns", "total_ns")
        out = {k: int(a[i]) for i, k in enumerate(names) if k}
        out["rounds"], out["tail_rounds"] = int(a[5]) & 0xFFFFFFFF, int(a[5]) >> 32
        out["wave_rows"], out["workgroup_rows"] = int(a[6]) & 0xFFFFFFFF, int(a[6]) >> 32
        return out

    def greedy_degree_last_path(self):
        """rtc_greedy_degree_last_path: DEGREE_PATH_WAVE | DEGREE_PATH_WORKGROUP | DEGREE_PATH_TAIL of the last greedy_degree call"""
        return int(self.lib.rtc_greedy_degree_last_path(self.h))

    def tree_medoids(self, n, edges, dedup_dist, seq_len=None, threads=None):
        """--dedup-dist representatives (build_dedup_candidates_per_cluster_core): node_to_rep[n] (int32) from forest edges
        (EDGE_DT records) -- each group of edges with dist <= dedup_dist represented by its tree medoid.  threads: host
        threads of the small groups (rtc_ctx_set_host_threads).  RTC_DEDUP_GPU picks the path (see dedup_last_path)."""
        e = np.ascontiguousarray(np.asarray(edges, dtype=EDGE_DT))
        lens = None if seq_len is None else np.ascontiguousarray(np.asarray(seq_len, dtype=np.uint64))
        if lens is not None and lens.shape[0] != n:
            raise ValueError("seq_len must hold n values")
        if threads is not None:
            self.check(self.lib.rtc_ctx_set_host_threads(self.h, int(threads)))
        out = np.zeros(max(int(n), 1), dtype=np.int32)
        self.check(self.lib.rtc_tree_medoids(self.h, int(n), _np_ptr(e) if len(e) else None, len(e), float(dedup_dist),
                                             _np_ptr(lens) if lens is not None else None, _np_ptr(out)))
        return out[:n].copy()

    def dedup_last_path(self):
        """Where the last tree_medoids call computed its sums: 0 nowhere, 1 host, 2 GPU, 3 both."""
        return int(self.lib.rtc_dedup_last_path(self.h))

    def rep_match(self, sk, n_reps, threshold, is_kssd=False, is_containment=False, query_chunk=0):
        """clust-mst --append against a stored state: sk holds the n_reps representatives, then the queries.  Returns the
        REP_PAIR_DT pairs (query, slot < n_reps + query, common, dist) that pass the reference's filters, sorted by (query,
        slot).  query_chunk > 0: that many queries per join (diag()["repmatch_chunks"] counts them)."""
        nq = sk.n - int(n_reps)
        if nq < 0:
            raise ValueError("n_reps exceeds the sketch set")
        cap = max(1024, 16 * max(nq, 1))
        while True:
            out = np.zeros(cap, dtype=REP_PAIR_DT)
            n = C.c_uint64()
            self.check(self.lib.rtc_rep_match(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len),
                                              int(n_reps), nq, sk.k, int(bool(is_kssd)), int(bool(is_containment)),
                                              float(threshold), int(query_chunk), _np_ptr(out), cap, C.byref(n)))
            if n.value <= cap:
                return out[:n.value].copy()
            cap = int(n.value)

    def rep_topk(self, sk, n_reps, wmode, topk, live=None, query_chunk=0):
        """clust-mst --db --query: sk holds the n_reps representatives, then the queries.  wmode: 0 set Jaccard, 1
        containment, 2 | s << 2 Mash's union-truncated estimator; topk 0 keeps every candidate.  live: n_reps flags (None:
        all live).  Returns (REP_HIT_DT records sorted by (query, rank), kept count per query as uint32)."""
        nq = sk.n - int(n_reps)
        if nq < 0:
            raise ValueError("n_reps exceeds the sketch set")
        lv = None
        if live is not None:
            lv = np.ascontiguousarray(np.asarray(live, dtype=np.uint8))
            if lv.shape != (int(n_reps),):
                raise ValueError("live needs one flag per representative")
        per = np.zeros(max(nq, 1), dtype=np.uint32)
        cap = max(1024, (int(topk) if topk else 16) * max(nq, 1))
        while True:
            out = np.zeros(cap, dtype=REP_HIT_DT)
            n = C.c_uint64()
            self.check(self.lib.rtc_rep_topk(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), int(n_reps), nq,
                                             _np_ptr(lv) if lv is not None else None, int(wmode), int(topk), int(query_chunk),
                                             _np_ptr(out), cap, C.byref(n), _np_ptr(per)))
            if n.value <= cap:
                return out[:n.value].copy(), per[:nq].copy()
            cap = int(n.value)

    def rep_topk_last_path(self):
        """Selection paths of the last rep_topk call: bit 0 one wave, bit 1 a 256-lane workgroup, bit 2 the host sort."""
        return int(self.lib.rtc_rep_topk_last_path(self.h))

    def rep_topk_counters(self):
        """rtc_rep_topk_counters as a dict (the last rep_topk call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_rep_topk_counters(self.h, a))
        names = ("chunks", "wave_queries", "workgroup_queries", "sort_queries", "candidates", "bytes_read", "join_ns",
                 "bucket_ns", "select_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def rep_screen(self, sk, n_reps, min_common=1, min_containment_q20=0, min_unique=1, max_picks=0, live=None, query_chunk=0):
        """clust-mst --db --screen: sk holds the n_reps representatives, then the samples (KSSD sketches).  Containment of every
        representative in every sample and the winner-takes-all decomposition of include/rtclust.h (rtc_rep_screen).
        min_containment_q20: round(min_containment * SCREEN_Q20), 0 for no containment test.  live: n_reps flags (None: all live).
        Returns (SCREEN_HIT_DT records sorted by query, picks first by rank, the rest by containment; SCREEN_SUM_DT, one per sample)."""
        nq = sk.n - int(n_reps)
        if nq < 0:
            raise ValueError("n_reps exceeds the sketch set")
        lv = None
        if live is not None:
            lv = np.ascontiguousarray(np.asarray(live, dtype=np.uint8))
            if lv.shape != (int(n_reps),):
                raise ValueError("live needs one flag per representative")
        sums = np.zeros(max(nq, 1), dtype=SCREEN_SUM_DT)
        cap = max(1024, 64 * max(nq, 1))
        while True:
            out = np.zeros(cap, dtype=SCREEN_HIT_DT)
            n = C.c_uint64()
            self.check(self.lib.rtc_rep_screen(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), int(n_reps), nq,
                                               _np_ptr(lv) if lv is not None else None, int(min_common), int(min_containment_q20),
                                               int(min_unique), int(max_picks), int(query_chunk), _np_ptr(out), cap, C.byref(n), _np_ptr(sums)))
            if n.value <= cap:
                return out[:n.value].copy(), sums[:nq].copy()
            cap = int(n.value)

    def rep_screen_last_path(self):
        """rtc_rep_screen_last_path: SCREEN_PATH_WAVE | SCREEN_PATH_BLOCK | SCREEN_PATH_GLOBAL, the gather paths of the last rep_screen call"""
        return int(self.lib.rtc_rep_screen_last_path(self.h))

    def rep_screen_counters(self):
        """rtc_rep_screen_counters as a dict (the last rep_screen call)."""
        a = (C.c_uint64 * 12)()
        self.check(self.lib.rtc_rep_screen_counters(self.h, a))
        names = ("chunks", "matches", "candidates", "eligible", "picks", "rounds_max", "wave_queries", "workgroup_queries", "global_queries",
                 "expand_ns", "gather_ns", "call_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def dbscan(self, sk, eps, min_pts, kmer_size, max_posting=0, return_core=False):
        """clust-dbscan --fast (KssdDBSCAN, src/dbscan.cpp:725-985) on the sketch set: int32 label per point, clusters numbered
        in the reference's order, -1 for noise.  kmer_size: the k of exp(-eps k) (from genomes the tuned k, from a sketch folder
        half_k * 2).  return_core: (labels, bool core flags)."""
        n = sk.n
        labels = np.zeros(max(n, 1), dtype=np.int32)
        core = np.zeros(max(n, 1), dtype=np.uint8)
        ncl, nnoise = C.c_uint32(), C.c_uint32()
        self.check(self.lib.rtc_dbscan(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, float(eps),
                                       int(min_pts), int(kmer_size), int(max_posting), _np_ptr(labels), _np_ptr(core),
                                       C.byref(ncl), C.byref(nnoise)))
        if return_core:
            return labels[:n].copy(), core[:n].astype(bool)
        return labels[:n].copy()

    def dbscan_knn(self, sk, eps, min_pts, kmer_size, knn_k, max_posting=0, return_core=False):
        """clust-dbscan --fast --knn K (rtc_dbscan_knn): KssdDBSCAN over the reference's k-NN graph (src/dbscan.cpp:221-360,
        :444-454), whose neighbour relation is directed; labels as Context.dbscan's.  knn_k <= 0 and u64 sketches are
        Context.dbscan's call; knn_k < min_pts - 1 is raised to it.  return_core: (labels, bool core flags)."""
        n = sk.n
        labels = np.zeros(max(n, 1), dtype=np.int32)
        core = np.zeros(max(n, 1), dtype=np.uint8)
        ncl, nnoise = C.c_uint32(), C.c_uint32()
        self.check(self.lib.rtc_dbscan_knn(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, float(eps),
                                           int(min_pts), int(kmer_size), int(max_posting), int(knn_k), _np_ptr(labels),
                                           _np_ptr(core), C.byref(ncl), C.byref(nnoise)))
        self.dbscan_knn_counts = (int(ncl.value), int(nnoise.value))
        if return_core:
            return labels[:n].copy(), core[:n].astype(bool)
        return labels[:n].copy()

    def dbscan_knn_counters(self):
        """rtc_dbscan_knn_counters as a dict (the last dbscan_knn call), with propagate_ns (rtc_dbscan_knn_propagate_ns)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_dbscan_knn_counters(self.h, a))
        names = ("chunks", "candidate_edges", "passers", "truncated_rows", "arrival_rows", "neighbour_edges", "core_points",
                 "rounds", "select_ns", "total_ns")
        out = {k: int(a[i]) for i, k in enumerate(names)}
        out["propagate_ns"] = int(self.lib.rtc_dbscan_knn_propagate_ns(self.h))
        return out

    def dbscan_sweep(self, sk, eps_list, min_pts, kmer_size, max_posting=0, return_core=False, kdist=False):
        """clust-dbscan --eps-sweep / --kdist (rtc_dbscan_sweep): Context.dbscan for every eps of eps_list (at most 32, any order)
        from one pair phase.  Returns int32 labels[n_eps, n]; with return_core also bool core[n_eps, n]; with kdist also the
        k-distance curve, KDIST_CURVE_DT per point (k = min_pts - 1; neighbour KDIST_NONE and distance inf where a point has
        fewer than k candidates).  An empty eps_list with kdist=True computes the curve alone.  The call's cluster and noise
        counts per eps stay in self.dbscan_sweep_counts."""
        n = sk.n
        eps = np.ascontiguousarray(np.asarray(list(eps_list), dtype=np.float64))
        L = int(eps.size)
        labels = np.zeros((L, n), dtype=np.int32)
        core = np.zeros((L, n), dtype=np.uint8)
        ncl, nnoise = np.zeros(max(L, 1), dtype=np.uint32), np.zeros(max(L, 1), dtype=np.uint32)
        kd = np.zeros(max(n, 1), dtype=KDIST_DT) if kdist else None
        buf_l = labels if labels.size else np.zeros(1, dtype=np.int32)
        buf_c = core if core.size else np.zeros(1, dtype=np.uint8)
        self.check(self.lib.rtc_dbscan_sweep(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, _np_ptr(eps) if L else None,
                                             L, int(min_pts), int(kmer_size), int(max_posting), _np_ptr(buf_l), _np_ptr(buf_c),
                                             _np_ptr(ncl), _np_ptr(nnoise), _np_ptr(kd) if kdist else None))
        self.dbscan_sweep_counts = {"clusters": ncl[:L].copy(), "noise": nnoise[:L].copy()}
        out = [labels]
        if return_core:
            out.append(core.astype(bool))
        if kdist:
            curve = np.zeros(n, dtype=KDIST_CURVE_DT)
            for f in KDIST_DT.names:
                curve[f] = kd[f][:n]
            cols = [kd[f][:n].tolist() for f in KDIST_DT.names]  # plain ints: a record at a time is slow at 200 000 points
            curve["distance"] = [math.inf if q == KDIST_NONE else kdist_distance(c, a, b, kmer_size) for c, a, b, q in zip(*cols)]
            out.append(curve)
        return out[0] if len(out) == 1 else tuple(out)

    def dbscan_sweep_counters(self):
        """rtc_dbscan_sweep_counters as a dict (the last dbscan_sweep call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_dbscan_sweep_counters(self.h, a))
        names = ("chunks", "candidate_edges", "kept_edges", "levels", "hook_rounds", "pair_ns", "predicate_ns", "components_ns",
                 "kdist_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def dbscan_mash(self, sk, sketch_size, eps_list, min_pts, kmer_size, return_core=False):
        """clust-dbscan --minhash (rtc_dbscan_mash): MinHashDBSCAN (src/dbscan.cpp:987-1096) over MinHash sketches of at most
        sketch_size hashes for every eps of eps_list (1 to 32 values in [0, 1), any order) from one pair phase.  A point is a core
        point with at least min_pts neighbours, itself not counted.  Returns int32 labels[n_eps, n] (-1 noise); with return_core
        also bool core[n_eps, n].  The call's cluster and noise counts per eps stay in self.dbscan_mash_counts."""
        n = sk.n
        eps = np.ascontiguousarray(np.asarray(list(eps_list), dtype=np.float64))
        L = int(eps.size)
        labels = np.zeros((L, n), dtype=np.int32)
        core = np.zeros((L, n), dtype=np.uint8)
        ncl, nnoise = np.zeros(max(L, 1), dtype=np.uint32), np.zeros(max(L, 1), dtype=np.uint32)
        buf_l = labels if labels.size else np.zeros(1, dtype=np.int32)
        buf_c = core if core.size else np.zeros(1, dtype=np.uint8)
        self.check(self.lib.rtc_dbscan_mash(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, int(sketch_size),
                                            _np_ptr(eps) if L else None, L, int(min_pts), int(kmer_size), _np_ptr(buf_l), _np_ptr(buf_c),
                                            _np_ptr(ncl), _np_ptr(nnoise)))
        self.dbscan_mash_counts = {"clusters": ncl[:L].copy(), "noise": nnoise[:L].copy()}
        return (labels, core.astype(bool)) if return_core else labels

    def dbscan_mash_counters(self):
        """rtc_dbscan_mash_counters as a dict (the last dbscan_mash call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_dbscan_mash_counters(self.h, a))
        names = ("chunks", "candidate_edges", "merged", "kept_edges", "levels", "hook_rounds", "pair_ns", "predicate_ns",
                 "components_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def dbscan_assign(self, sk, n_db, labels, core, eps, min_pts, kmer_size, sketch_size=None, query_chunk=0):
        """clust-dbscan --db --assign (rtc_dbscan_assign): sk holds the n_db model points, then the queries; labels / core are the
        model's, from Context.dbscan (sketch_size None) or Context.dbscan_mash (sketch_size: the estimator's) at this eps,
        min_pts and kmer_size.  Returns PLACE_DT per query: label / label_max (-1: novel; different: a bridge), n_neighbours,
        n_core, nearest (PLACE_NONE: no shared hash) with its common / denom, flags (bit 0: would be a core point)."""
        nq = sk.n - int(n_db)
        if nq < 0:
            raise ValueError("n_db exceeds the sketch set")
        lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, dtype=np.int32))
        cr = None if core is None else np.ascontiguousarray(np.asarray(core, dtype=np.uint8))
        if (lab is not None and lab.shape != (int(n_db),)) or (cr is not None and cr.shape != (int(n_db),)):
            raise ValueError("labels and core need one entry per model point")
        out = np.zeros(max(nq, 1), dtype=PLACE_DT)
        self.check(self.lib.rtc_dbscan_assign(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), int(n_db), nq,
                                              _np_ptr(lab) if lab is not None else None, _np_ptr(cr) if cr is not None else None,
                                              0 if sketch_size is None else 1, 0 if sketch_size is None else int(sketch_size),
                                              float(eps), int(min_pts), int(kmer_size), int(query_chunk), _np_ptr(out)))
        return out[:nq].copy()

    def dbscan_assign_counters(self):
        """rtc_dbscan_assign_counters as a dict (the last dbscan_assign call); fold_paths: bit 0 one wave per query, bit 1 a
        256-lane workgroup (rtc_dbscan_assign_last_path)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_dbscan_assign_counters(self.h, a))
        names = ("chunks", "candidates", "neighbours", "placed", "novel", "bridging", "join_ns", "predicate_ns", "fold_ns", "total_ns")
        out = {k: int(a[i]) for i, k in enumerate(names)}
        out["fold_paths"] = int(self.lib.rtc_dbscan_assign_last_path(self.h))
        return out

    def dbscan_update(self, sk, n_old, labels, core, eps, min_pts, kmer_size, sketch_size=None):
        """clust-dbscan --db --update (rtc_dbscan_update): sk holds the n_old model points, then the new ones; labels / core are
        the model's, from Context.dbscan (sketch_size None) or Context.dbscan_mash (sketch_size: the estimator's) at this eps,
        min_pts and kmer_size.  Returns (labels, bool core) over all of sk, equal to that call on all of sk; only the new rows and
        the old noise and border rows that can change are joined.  The cluster and noise counts stay in self.dbscan_update_counts."""
        n_old, n = int(n_old), sk.n
        if n_old > n:
            raise ValueError("n_old exceeds the sketch set")
        lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, dtype=np.int32))
        cr = None if core is None else np.ascontiguousarray(np.asarray(core, dtype=np.uint8))
        if (lab is not None and lab.shape != (n_old,)) or (cr is not None and cr.shape != (n_old,)):
            raise ValueError("labels and core need one entry per model point")
        out_l = np.zeros(max(n, 1), dtype=np.int32)
        out_c = np.zeros(max(n, 1), dtype=np.uint8)
        ncl, nnoise = C.c_uint32(), C.c_uint32()
        self.check(self.lib.rtc_dbscan_update(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n_old, n - n_old,
                                              _np_ptr(lab) if lab is not None else None, _np_ptr(cr) if cr is not None else None,
                                              0 if sketch_size is None else 1, 0 if sketch_size is None else int(sketch_size),
                                              float(eps), int(min_pts), int(kmer_size), _np_ptr(out_l), _np_ptr(out_c),
                                              C.byref(ncl), C.byref(nnoise)))
        self.dbscan_update_counts = (int(ncl.value), int(nnoise.value))
        return out_l[:n].copy(), out_c[:n].astype(bool)

    def dbscan_update_counters(self):
        """rtc_dbscan_update_counters as a dict (the last dbscan_update call)."""
        a = (C.c_uint64 * 12)()
        self.check(self.lib.rtc_dbscan_update_counters(self.h, a))
        names = ("stage1_rows", "stage2_rows", "chunks", "candidate_edges", "kept_edges", "promoted", "merged", "hook_rounds",
                 "join_ns", "predicate_ns", "components_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def dbscan_hierarchy(self, sk, eps_max, min_pts, kmer_size, max_posting=0):
        """clust-dbscan --hierarchy (rtc_dbscan_hierarchy): the maximum spanning forest of the mutual-reachability relation over
        the pairs Context.dbscan keeps at eps_max, and every point's core triple.  Returns (forest, core): HEDGE_DT edges in the
        total order (larger m first, then smaller p, then smaller q) and KDIST_DT per point, which is dbscan_sweep's k-distance
        curve.  hierarchy_cut / hierarchy_flat read both."""
        n = sk.n
        forest = np.zeros(max(n, 1), dtype=HEDGE_DT)
        core = np.zeros(max(n, 1), dtype=KDIST_DT)
        nf = C.c_uint64(0)
        self.check(self.lib.rtc_dbscan_hierarchy(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, float(eps_max),
                                                 int(min_pts), int(kmer_size), int(max_posting), _np_ptr(forest), C.byref(nf), _np_ptr(core)))
        return forest[:nf.value].copy(), core[:n].copy()

    def dbscan_sweep_hierarchy(self, sk, eps_list, eps_max, min_pts, kmer_size, max_posting=0):
        """rtc_dbscan_sweep_hierarchy: dbscan_sweep(eps_list, return_core=True) and dbscan_hierarchy(eps_max) from ONE pair phase
        (what clust-dbscan --hierarchy --eps-sweep runs).  Returns (labels[n_eps, n], bool core flags[n_eps, n], forest, core
        triples), each exactly as from its own call; both counter sets are filled."""
        n = sk.n
        eps = np.ascontiguousarray(np.asarray(list(eps_list), dtype=np.float64))
        L = int(eps.size)
        labels = np.zeros((L, n), dtype=np.int32)
        flags = np.zeros((L, n), dtype=np.uint8)
        ncl, nnoise = np.zeros(max(L, 1), dtype=np.uint32), np.zeros(max(L, 1), dtype=np.uint32)
        buf_l = labels if labels.size else np.zeros(1, dtype=np.int32)
        buf_c = flags if flags.size else np.zeros(1, dtype=np.uint8)
        forest = np.zeros(max(n, 1), dtype=HEDGE_DT)
        core = np.zeros(max(n, 1), dtype=KDIST_DT)
        nf = C.c_uint64(0)
        self.check(self.lib.rtc_dbscan_sweep_hierarchy(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n,
                                                       _np_ptr(eps) if L else None, L, int(min_pts), int(kmer_size), int(max_posting),
                                                       _np_ptr(buf_l), _np_ptr(buf_c), _np_ptr(ncl), _np_ptr(nnoise), None, float(eps_max),
                                                       _np_ptr(forest), C.byref(nf), _np_ptr(core)))
        self.dbscan_sweep_counts = {"clusters": ncl[:L].copy(), "noise": nnoise[:L].copy()}
        return labels, flags.astype(bool), forest[:nf.value].copy(), core[:n].copy()

    def dbscan_hierarchy_counters(self):
        """rtc_dbscan_hierarchy_counters as a dict (the last hierarchy call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_dbscan_hierarchy_counters(self.h, a))
        names = ("chunks", "candidate_edges", "kept_edges", "forest_edges", "boruvka_rounds", "pair_ns", "kdist_ns", "rank_ns",
                 "forest_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def graph_build(self, sk, threshold, kmer_size, knn_k=0, cap=None):
        """clust-leiden's similarity graph (rtc_graph_build; KssdLeidenCluster, src/leiden.cpp:168-293): GEDGE_DT edges (u < v,
        common) in (u, v) order.  knn_k > 0: every node keeps its knn_k best edges among the higher-numbered neighbours.  cap:
        room for the edges (None: the call is repeated with the count it reports); an explicit cap that is too small raises
        RTC_ERR_OVERFLOW, the needed count in self.graph_edges_needed."""
        n = sk.n
        room = max(int(cap) if cap is not None else 16 * n, 1)
        while True:
            out = np.zeros(room, dtype=GEDGE_DT)
            ne = C.c_uint64(0)
            st = self.lib.rtc_graph_build(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, float(threshold),
                                          int(kmer_size), int(knn_k), _np_ptr(out), int(cap) if cap is not None else room, C.byref(ne))
            self.graph_edges_needed = int(ne.value)
            if st == _lib.RTC_ERR_OVERFLOW and cap is None:
                room = int(ne.value)
                continue
            self.check(st)
            return out[:ne.value].copy()

    def graph_build_mash(self, sk, sketch_size, threshold, kmer_size, knn_k=0, cap=None):
        """clust-leiden --minhash's similarity graph (rtc_graph_build_mash): GEDGE_DT edges (u < v, common) in (u, v) order over
        MinHash sketches of at most sketch_size hashes; a pair is an edge iff rtc_mash_distance(common, denom) < threshold, on
        the union-truncated counts.  The field `pad` holds the truncated denom (graph_denom(edges)).  knn_k and cap as
        graph_build: the rank is common / denom."""
        n = sk.n
        room = max(int(cap) if cap is not None else 16 * n, 1)
        while True:
            out = np.zeros(room, dtype=GEDGE_DT)
            ne = C.c_uint64(0)
            st = self.lib.rtc_graph_build_mash(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, int(sketch_size),
                                               float(threshold), int(kmer_size), int(knn_k), _np_ptr(out), int(cap) if cap is not None else room,
                                               C.byref(ne))
            self.graph_edges_needed = int(ne.value)
            if st == _lib.RTC_ERR_OVERFLOW and cap is None:
                room = int(ne.value)
                continue
            self.check(st)
            return out[:ne.value].copy()

    def graph_counters(self):
        """rtc_graph_counters as a dict (the last graph_build or graph_build_mash call; merged: the candidates merged past the
        prefilter of a MinHash call, 0 after graph_build)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_graph_counters(self.h, a))
        names = ("chunks", "candidates", "passing", "edges", "nodes_cut", "pair_ns", "filter_ns", "select_ns", "merged", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def louvain(self, n, edges, resolution=1.0, return_modularity=False):
        """rtc_louvain: the deterministic Louvain include/rtclust.h defines over n vertices and WEDGE_DT records (u, v, q), q the
        weight in units of 2^-20 (graph_weights forms them).  Returns int32 labels, communities numbered by their smallest
        vertex; with return_modularity (labels, modularity)."""
        e = np.ascontiguousarray(np.asarray(edges, dtype=WEDGE_DT))
        labels = np.zeros(max(int(n), 1), dtype=np.int32)
        ncl, mod = C.c_uint32(0), C.c_double(0.0)
        self.check(self.lib.rtc_louvain(self.h, int(n), _np_ptr(e) if e.size else None, int(e.size), float(resolution), _np_ptr(labels),
                                        C.byref(ncl), C.byref(mod)))
        self.louvain_clusters = int(ncl.value)
        return (labels[:n].copy(), float(mod.value)) if return_modularity else labels[:n].copy()

    def louvain_counters(self):
        """rtc_louvain_counters as a dict (the last louvain call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_louvain_counters(self.h, a))
        names = ("levels", "rounds", "moves", "last_vertices", "last_entries", "long_rows", "move_ns", "aggregate_ns", "global_rows",
                 "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def leiden(self, n, edges, resolution=1.0, objective="cpm", return_quality=False):
        """rtc_leiden: the deterministic Leiden include/rtclust.h defines over n vertices and WEDGE_DT records (u, v, q).
        objective "cpm" (node weight 1, as the reference calls igraph; at resolution >= 1 and weights of at most one unit nothing
        moves) or "modularity"; 0 and 1 are taken too.  Returns int32 labels, communities numbered by their smallest vertex; with
        return_quality (labels, quality)."""
        obj = {"cpm": 0, "modularity": 1}.get(objective, objective)
        e = np.ascontiguousarray(np.asarray(edges, dtype=WEDGE_DT))
        labels = np.zeros(max(int(n), 1), dtype=np.int32)
        ncl, quality = C.c_uint32(0), C.c_double(0.0)
        self.check(self.lib.rtc_leiden(self.h, int(n), _np_ptr(e) if e.size else None, int(e.size), float(resolution), int(obj),
                                       _np_ptr(labels), C.byref(ncl), C.byref(quality)))
        self.leiden_clusters = int(ncl.value)
        return (labels[:n].copy(), float(quality.value)) if return_quality else labels[:n].copy()

    def leiden_counters(self):
        """rtc_leiden_counters as a dict (the last leiden call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_leiden_counters(self.h, a))
        names = ("iterations", "levels", "move_rounds", "moves", "refine_rounds", "merges", "rejected", "move_ns", "refine_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def mcl(self, n, edges, inflation=2.0, select=1024, max_iter=100, return_matrix=False):
        """rtc_mcl: the Markov clustering include/rtclust.h defines in fixed point over n vertices and WEDGE_DT records (u, v, q).
        inflation: a multiple of 0.5 from 1.5 to 8 (the library takes twice the value as an integer).  Returns int32 labels, every
        vertex labelled by the smallest member of its cluster; with return_matrix (labels, matrix), the final matrix as
        MCL_ENTRY_DT records in (col, row) order.  mcl_iterations, mcl_converged and mcl_clusters hold the rest of the result."""
        h = int(round(float(inflation) * 2))
        if h != float(inflation) * 2:
            raise ValueError(f"inflation {inflation} is no multiple of 0.5")
        e = np.ascontiguousarray(np.asarray(edges, dtype=WEDGE_DT))
        labels = np.zeros(max(int(n), 1), dtype=np.int32)
        ncl, its, nnz, conv = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_int(0)

        def call(mat):
            return self.lib.rtc_mcl(self.h, int(n), _np_ptr(e) if e.size else None, int(e.size), h, int(select), int(max_iter), _np_ptr(labels),
                                    C.byref(ncl), C.byref(its), C.byref(conv), _np_ptr(mat) if mat is not None else None,
                                    int(mat.size) if mat is not None else 0, C.byref(nnz))
        mat = None
        if return_matrix:  # room for what the columns can hold, up to 64 MiB; a larger matrix names its size and the call is repeated
            mat = np.zeros(max(min(int(n) * min(int(select), max(int(n), 1)), 1 << 22), 1), dtype=MCL_ENTRY_DT)
        st = call(mat)
        if st == _lib.RTC_ERR_OVERFLOW and return_matrix and int(nnz.value) > mat.size:
            mat = np.zeros(int(nnz.value), dtype=MCL_ENTRY_DT)
            st = call(mat)
        self.check(st)
        self.mcl_clusters, self.mcl_iterations, self.mcl_converged = int(ncl.value), int(its.value), int(conv.value)
        return (labels[:n].copy(), mat[:int(nnz.value)].copy()) if return_matrix else labels[:n].copy()

    def mcl_counters(self):
        """rtc_mcl_counters as a dict (the last mcl call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_mcl_counters(self.h, a))
        names = ("iterations", "converged", "entries", "attractors", "wave_columns", "workgroup_columns", "global_columns", "cut_columns",
                 "expand_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def mcl_last_path(self):
        """rtc_mcl_last_path: MCL_PATH_WAVE | MCL_PATH_WORKGROUP | MCL_PATH_GLOBAL, the column paths of the last mcl call"""
        return int(self.lib.rtc_mcl_last_path(self.h))

    def graph_snn(self, n, u, v):
        """rtc_graph_snn: the shared-neighbour counts include/rtclust.h defines over n vertices and the records (u[e], v[e]).
        Returns (shared, deg_u, deg_v, flags), uint32 arrays with one entry per record; snn_weight turns them into weights."""
        u = np.asarray(u, dtype=np.uint32).reshape(-1)
        v = np.asarray(v, dtype=np.uint32).reshape(-1)
        if u.shape != v.shape:
            raise ValueError("u and v must hold one entry per record")
        e = np.zeros(u.size, dtype=WEDGE_DT)
        e["u"], e["v"] = u, v
        out = np.zeros(max(int(e.size), 1), dtype=SNN_DT)
        self.check(self.lib.rtc_graph_snn(self.h, int(n), _np_ptr(e) if e.size else None, int(e.size), _np_ptr(out) if e.size else None))
        out = out[:e.size]
        return out["shared"].copy(), out["deg_u"].copy(), out["deg_v"].copy(), out["flags"].copy()

    def graph_snn_counters(self):
        """rtc_graph_snn_counters as a dict (the last graph_snn call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_graph_snn_counters(self.h, a))
        names = ("records", "edges", "triangles", "probes", "wave_records", "workgroup_records", "global_records", "adjacency_ns",
                 "count_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def graph_snn_last_path(self):
        """rtc_graph_snn_last_path: SNN_PATH_WAVE | SNN_PATH_WORKGROUP | SNN_PATH_GLOBAL, the paths of the last graph_snn call"""
        return int(self.lib.rtc_graph_snn_last_path(self.h))

    def silhouette(self, n, edges, labels):
        """rtc_silhouette: the score include/rtclust.h defines over n vertices, WEDGE_DT records (u, v, q) -- q the distance of the
        pair in units of 2^-20, unlisted pairs at SIL_ONE -- and one int32 label per vertex, negative for an unclustered one.
        Returns SIL_DT records, one per vertex; silhouette_value turns them into the silhouette."""
        e = np.ascontiguousarray(np.asarray(edges, dtype=WEDGE_DT))
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32))
        if lab.shape != (int(n),):
            raise ValueError("labels must hold one label per vertex")
        out = np.zeros(max(int(n), 1), dtype=SIL_DT)
        self.check(self.lib.rtc_silhouette(self.h, int(n), _np_ptr(e) if e.size else None, int(e.size), _np_ptr(lab) if n else None,
                                           _np_ptr(out) if n else None))
        return out[:int(n)].copy()

    def silhouette_counters(self):
        """rtc_silhouette_counters as a dict (the last silhouette call, or the score of the last cluster_quality call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_silhouette_counters(self.h, a))
        names = ("records", "entries", "clustered", "clusters", "wave_rows", "workgroup_rows", "global_rows", "csr_ns", "rows_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def silhouette_last_path(self):
        """rtc_silhouette_last_path: SIL_PATH_WAVE | SIL_PATH_WORKGROUP | SIL_PATH_GLOBAL, the row paths of the last score"""
        return int(self.lib.rtc_silhouette_last_path(self.h))

    def cluster_quality(self, sk, labels, kmer_size):
        """rtc_cluster_quality: rtc_silhouette over sk's sketches, every pair that shares a hash at the distance
        rtc_linkage_distance gives its exact key, every other pair at 1.  labels: one int32 per sketch from any algorithm -- the
        MST's cut, ctx.louvain(...)'s communities, a DBSCAN run's labels with -1 for noise.  Returns SIL_DT records."""
        n = sk.n
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32))
        if lab.shape != (n,):
            raise ValueError("labels must hold one label per sketch")
        out = np.zeros(max(n, 1), dtype=SIL_DT)
        self.check(self.lib.rtc_cluster_quality(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, _np_ptr(lab),
                                                int(kmer_size), _np_ptr(out)))
        return out[:n].copy()

    def cluster_quality_counters(self):
        """rtc_cluster_quality_counters as a dict (the last cluster_quality call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_cluster_quality_counters(self.h, a))
        names = ("chunks", "candidates", "wave_rows", "workgroup_rows", "global_rows", "pair_ns", "distance_ns", "score_ns", "clusters",
                 "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def linkage(self, keys, kmin=(0, 1)):
        """rtc_linkage_dev: the complete-linkage agglomeration include/rtclust.h defines over one symmetric m x m key matrix --
        an array [m, m, 2] of (common, denom), or LKEY_DT [m, m] -- uploaded for the call.  kmin: the stop bound (num, den),
        (0, 1) none.  Returns LMERGE_DT records (a, b, common, denom, size) in step order, a and b as matrix indices."""
        k = np.ascontiguousarray(keys)
        if k.dtype == LKEY_DT:
            k = k.view(np.uint32).reshape(k.shape + (2,))
        k = np.ascontiguousarray(k, dtype=np.uint32)
        m = int(k.shape[0])
        if k.ndim != 3 or k.shape[1] != m or k.shape[2] != 2:
            raise ValueError("keys must be [m, m, 2]")
        d = torch.from_numpy(k.view(np.int32).reshape(-1).copy()).to(self.device) if m else torch.zeros(2, dtype=torch.int32, device=self.device)
        out = np.zeros(max(m - 1, 1), dtype=LMERGE_DT)
        nm = C.c_uint32(0)
        self.check(self.lib.rtc_linkage_dev(self.h, m, _t_ptr(d), m, int(kmin[0]), int(kmin[1]), _np_ptr(out), C.byref(nm)))
        return out[:nm.value].copy()

    def linkage_complete(self, sk, comp, kmin=(0, 1), cap=None):
        """rtc_linkage_complete: the agglomeration inside every component of the labelling comp[g] of sk's sketches (any labels;
        components are numbered by their smallest member).  Returns (merges, first): LMERGE_DT records with a and b as genome
        indices, component after component, and first[c] where component c's merges start (len(first) - 1 components).  cap:
        room for the merges (None: n - 1, which always suffices); too small raises RTC_ERR_OVERFLOW, the needed count in
        self.linkage_merges_needed."""
        n = sk.n
        lab = np.ascontiguousarray(np.asarray(comp).astype(np.int64).astype(np.uint32))
        if lab.shape != (n,):
            raise ValueError("comp must hold one label per sketch")
        room = max(n - 1, 1) if cap is None else int(cap)
        out = np.zeros(max(room, 1), dtype=LMERGE_DT)
        first = np.zeros(n + 1, dtype=np.uint64)
        nm = C.c_uint64(0)
        st = self.lib.rtc_linkage_complete(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, _np_ptr(lab),
                                           int(kmin[0]), int(kmin[1]), _np_ptr(out), room, C.byref(nm), _np_ptr(first))
        self.linkage_merges_needed = int(nm.value)
        self.check(st)
        return out[:nm.value].copy(), first[:len(np.unique(lab)) + 1].copy()

    def linkage_counters(self):
        """rtc_linkage_counters as a dict (the last linkage or linkage_complete call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_linkage_counters(self.h, a))
        names = ("components", "wave_components", "workgroup_components", "merges", "rescans", "batches", "fill_ns", "agglomerate_ns",
                 "largest_m", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def nj(self, matrix, ld=None):
        """rtc_nj_dev: the neighbour joining include/rtclust.h defines over one symmetric m x m matrix of doubles, uploaded for the
        call.  ld: the row stride when the array is [m, ld] with ld > m.  Returns NJOIN_DT records in step order, a, b and c as
        matrix indices (c is 0xFFFFFFFF but in the last record of m >= 3)."""
        d = np.ascontiguousarray(matrix, dtype=np.float64)
        m = int(d.shape[0])
        ld = int(d.shape[1]) if d.ndim == 2 and m else m
        if d.ndim != 2 or ld < m:
            raise ValueError("matrix must be [m, ld] with ld >= m")
        t = torch.from_numpy(d.reshape(-1).copy()).to(self.device) if m else torch.zeros(2, dtype=torch.float64, device=self.device)
        out = np.zeros(max(m - 2, 1), dtype=NJOIN_DT)
        nj = C.c_uint32(0)
        self.check(self.lib.rtc_nj_dev(self.h, m, _t_ptr(t), ld, _np_ptr(out), C.byref(nj)))
        return out[:nj.value].copy()

    def nj_clusters(self, sk, comp, kmer_size, cap=None):
        """rtc_nj_clusters: one neighbour-joining tree per component of the labelling comp[g] of sk's sketches (any labels;
        components are numbered by their smallest member) over rtc_linkage_distance of the exact keys.  Returns (joins, first):
        NJOIN_DT records with a, b and c as genome indices, component after component, and first[c] where component c's records
        start.  cap: room for the records (None: n, which always suffices); too small raises RTC_ERR_OVERFLOW, the needed count
        in self.nj_records_needed."""
        n = sk.n
        lab = np.ascontiguousarray(np.asarray(comp).astype(np.int64).astype(np.uint32))
        if lab.shape != (n,):
            raise ValueError("comp must hold one label per sketch")
        room = max(n, 1) if cap is None else int(cap)
        out = np.zeros(max(room, 1), dtype=NJOIN_DT)
        first = np.zeros(n + 1, dtype=np.uint64)
        nj = C.c_uint64(0)
        st = self.lib.rtc_nj_clusters(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, _np_ptr(lab), int(kmer_size),
                                      _np_ptr(out), room, C.byref(nj), _np_ptr(first))
        self.nj_records_needed = int(nj.value)
        self.check(st)
        return out[:nj.value].copy(), first[:len(np.unique(lab)) + 1].copy()

    def nj_counters(self):
        """rtc_nj_counters as a dict (the last nj or nj_clusters call), and "paths": rtc_nj_last_path's bits."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_nj_counters(self.h, a))
        names = ("components", "wave_components", "workgroup_components", "grid_components", "records", "batches", "fill_ns", "distance_ns",
                 "join_ns", "total_ns")
        out = {k: int(a[i]) for i, k in enumerate(names)}
        out["paths"] = int(self.lib.rtc_nj_last_path(self.h))
        return out

    def nj_scan_blocks(self):
        """rtc_nj_scan_blocks: RTC_NJ_SCAN_BLOCKS as the context holds it, 1 .. NJ_SCAN_BLOCKS (unset: NJ_SCAN_BLOCKS)"""
        return int(self.lib.rtc_nj_scan_blocks(self.h))

    def nj_support(self, sk, comp, kmer_size, replicates, seed=0, cap=None):
        """rtc_nj_support: nj_clusters' (joins, first) for the same arguments and, third, one uint32 per record: how many of the
        `replicates` (1 .. NJ_SUPPORT_MAX) delete-half jackknife replicates over the sketch hashes hold the record's split; 0 for
        the records that name none (the closing one, and trees of three members or fewer).  nj_counters describes the main trees,
        nj_support_counters the replicates."""
        n = sk.n
        lab = np.ascontiguousarray(np.asarray(comp).astype(np.int64).astype(np.uint32))
        if lab.shape != (n,):
            raise ValueError("comp must hold one label per sketch")
        room = max(n, 1) if cap is None else int(cap)
        out = np.zeros(max(room, 1), dtype=NJOIN_DT)
        support = np.zeros(max(room, 1), dtype=np.uint32)
        first = np.zeros(n + 1, dtype=np.uint64)
        nj = C.c_uint64(0)
        st = self.lib.rtc_nj_support(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, _np_ptr(lab), int(kmer_size),
                                     int(replicates), int(seed) & 0xFFFFFFFFFFFFFFFF, _np_ptr(out), room, C.byref(nj), _np_ptr(first),
                                     _np_ptr(support))
        self.nj_records_needed = int(nj.value)
        self.check(st)
        return out[:nj.value].copy(), first[:len(np.unique(lab)) + 1].copy(), support[:nj.value].copy()

    def nj_support_counters(self):
        """rtc_nj_support_counters as a dict (the last nj_support call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_nj_support_counters(self.h, a))
        names = ("replicates", "replicate_trees", "count_ns", "distance_ns", "join_ns", "split_ns", "total_ns", "groups", "splits", "count_sum")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def jackknife_pairs(self, sk, pairs, seed=0, word=0, sizes=True):
        """rtc_jackknife_pairs_dev: the counting kernel's pair routine over the given pairs, an (m, 2) array of indices below sk.n.
        Returns (common, size): common[e, r] the hashes pair e shares that replicate 64 * word + r keeps, size[g, r] those of
        sketch g it keeps (None without sizes)."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        m = len(pairs)
        if m and (pairs.min() < 0 or pairs.max() >= sk.n):
            raise ValueError("jackknife_pairs: an index outside [0, n)")
        edges = np.zeros(max(m, 1), dtype=CEDGE_DT)
        edges["i"][:m], edges["j"][:m] = pairs[:, 0], pairs[:, 1]
        d_edges = torch.from_numpy(edges.view(np.uint32).reshape(-1, 3).view(np.int32)).to(self.device)
        common = torch.zeros((max(m, 1), 64), dtype=torch.int32, device=self.device)
        size = torch.zeros((max(sk.n, 1), 64), dtype=torch.int32, device=self.device) if sizes else None
        self.check(self.lib.rtc_jackknife_pairs_dev(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), sk.n, _t_ptr(d_edges), m,
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(word), _t_ptr(common), _t_ptr(size) if sizes else None))
        self.sync()
        return common[:m].cpu().numpy().view(np.uint32), (size[:sk.n].cpu().numpy().view(np.uint32) if sizes else None)

    def cluster_support(self, sk, comp, kmer_size, threshold, replicates, seed=0):
        """rtc_cluster_support: (records, together).  records: one CSUPPORT_DT per cluster of the labelling `comp` (any labelling),
        the clusters in order of their smallest member -- in how many of the `replicates` (1 .. CSUPPORT_MAX) delete-half jackknife
        replicates over the sketch hashes the cluster comes back whole and alone (recovered), in pieces (split), whole but joined
        to others (merged) or neither (mixed), and its most pieces.  together: one uint64 per sketch, the sum over the replicates
        of the genomes that stay with it, itself not counted."""
        n = sk.n
        lab = np.ascontiguousarray(np.asarray(comp).astype(np.int64).astype(np.uint32))
        if lab.shape != (n,):
            raise ValueError("comp must hold one label per sketch")
        n_cl = len(np.unique(lab))
        out = np.zeros(max(n_cl, 1), dtype=CSUPPORT_DT)
        together = np.zeros(max(n, 1), dtype=np.uint64)
        self.check(self.lib.rtc_cluster_support(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, _np_ptr(lab), int(kmer_size),
                                                float(threshold), int(replicates), int(seed) & 0xFFFFFFFFFFFFFFFF, _np_ptr(out), _np_ptr(together)))
        return out[:n_cl].copy(), together[:n].copy()

    def cluster_support_counters(self):
        """rtc_cluster_support_counters as a dict (the last cluster_support call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_cluster_support_counters(self.h, a))
        names = ("chunks", "candidates", "inner_kept", "crossing_kept", "hook_passes", "pair_ns", "count_ns", "components_ns", "tally_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def pangenome(self, sk, labels, soft_pct=95, cloud_pct=15):
        """rtc_pangenome: (clusters, hist, genomes).  labels[g] >= 0 is g's cluster (any number below n), negative: unclustered.
        clusters: one PAN_DT per cluster, the clusters in order of their smallest member -- size, total (the members' hashes), pan
        (distinct hashes), and those by class: core (held by every member), soft (by at least soft_pct % of them), cloud (by less
        than cloud_pct %), shell (the rest), and single (held by one).  hist: n uint64; cluster c owns the size_c entries behind
        those of the clusters before it, entry f - 1 the hashes held by f members.  genomes: one PAN_GENOME_DT per sketch -- its
        hashes nobody else in its cluster holds (unique), its hashes by class, and occ_sum, the sum over its hashes of the members
        that hold them."""
        n = sk.n
        lab = np.ascontiguousarray(np.asarray(labels).astype(np.int64).astype(np.int32))
        if lab.shape != (n,):
            raise ValueError("labels must hold one label per sketch")
        clusters = np.zeros(max(n, 1), dtype=PAN_DT)
        hist = np.zeros(max(n, 1), dtype=np.uint64)
        genomes = np.zeros(max(n, 1), dtype=PAN_GENOME_DT)
        n_cl = C.c_uint32(0)
        self.check(self.lib.rtc_pangenome(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, _np_ptr(lab), int(soft_pct),
                                          int(cloud_pct), _np_ptr(clusters), _np_ptr(hist), _np_ptr(genomes), C.byref(n_cl)))
        return clusters[:n_cl.value].copy(), hist[:n].copy(), genomes[:n].copy()

    def pangenome_counters(self):
        """rtc_pangenome_counters as a dict (the last pangenome call), with rtc_pangenome_phases' three times"""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_pangenome_counters(self.h, a))
        names = ("clusters", "clustered", "records", "distinct", "wave_clusters", "block_clusters", "global_clusters", "groups", "kernel_ns", "total_ns")
        out = {k: int(a[i]) for i, k in enumerate(names)}
        p = (C.c_uint64 * 3)()
        self.check(self.lib.rtc_pangenome_phases(self.h, p))
        out.update(count_ns=int(p[0]), sweep_ns=int(p[1]), genome_ns=int(p[2]))
        return out

    def pangenome_last_path(self):
        """the cluster paths of the last pangenome call: PAN_PATH_WAVE | PAN_PATH_BLOCK | PAN_PATH_GLOBAL"""
        return int(self.lib.rtc_pangenome_last_path(self.h))

    def components64(self, n, edges, masks, labels=None):
        """rtc_components64_dev: the connected components of 64 graphs over n vertices at once.  edges: an (m, 2) array of vertices
        below n, masks: m uint64 -- edge e belongs to graph r iff bit r of masks[e] is set.  labels: None for a fresh start, or
        the [n, 64] array an earlier call returned, to add these edges to those.  Returns labels[g, r], the smallest vertex of g's
        component in graph r, as uint32."""
        n = int(n)
        edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 2))
        mk = np.ascontiguousarray(np.asarray(masks, dtype=np.uint64).reshape(-1))
        m = len(edges)
        if len(mk) != m:
            raise ValueError("components64: one mask per edge")
        if m and (edges.min() < 0 or edges.max() >= n):
            raise ValueError("components64: a vertex outside [0, n)")
        if labels is None:
            lab = np.repeat(np.arange(n, dtype=np.uint32), 64).reshape(n, 64)
        else:
            lab = np.ascontiguousarray(np.asarray(labels, dtype=np.uint32))
            if lab.shape != (n, 64) or (n and (lab > np.arange(n, dtype=np.uint32)[:, None]).any()):
                raise ValueError("components64: labels must be [n, 64] and no label above its vertex")
        rec = np.zeros(max(m, 1), dtype=CEDGE_DT)
        rec["i"][:m], rec["j"][:m] = edges[:, 0], edges[:, 1]
        d_edges = torch.from_numpy(rec.view(np.uint32).reshape(-1, 3).view(np.int32)).to(self.device)
        d_mask = torch.from_numpy(np.concatenate([mk, np.zeros(1, dtype=np.uint64)]).view(np.int64)).to(self.device)
        d_lab = torch.from_numpy(np.concatenate([lab.reshape(-1), np.zeros(64, dtype=np.uint32)]).view(np.int32)).to(self.device)
        self.check(self.lib.rtc_components64_dev(self.h, n, _t_ptr(d_edges), _t_ptr(d_mask), m, _t_ptr(d_lab)))
        self.sync()
        return d_lab[:n * 64].cpu().numpy().view(np.uint32).reshape(n, 64)

    def upgma(self, sums, sizes=None, ld=None):
        """rtc_upgma_dev: the average-linkage agglomeration include/rtclust.h defines over one symmetric m x m matrix of uint64
        sums, uploaded for the call.  sizes: w[i] >= 1 per index (None: all 1).  ld: None takes the array as [m, ld]; a number
        is passed on as it is (the refusals).  Returns the m - 1 UMERGE_DT records in step order, a and b as matrix indices."""
        s = np.ascontiguousarray(sums, dtype=np.uint64)
        if s.ndim != 2:
            raise ValueError("sums must be [m, ld]")
        m = int(s.shape[0])
        ld = (int(s.shape[1]) if m else 0) if ld is None else int(ld)
        w = None if sizes is None else np.ascontiguousarray(sizes, dtype=np.uint32)
        if w is not None and w.shape != (m,):
            raise ValueError("sizes must hold one entry per row")
        t = torch.from_numpy(s.reshape(-1).view(np.int64).copy()).to(self.device) if s.size else torch.zeros(2, dtype=torch.int64, device=self.device)
        out = np.zeros(max(m - 1, 1), dtype=UMERGE_DT)
        self.check(self.lib.rtc_upgma_dev(self.h, m, _t_ptr(t), ld, None if w is None else _np_ptr(w), _np_ptr(out)))
        return out[:max(m - 1, 0)].copy()

    def upgma_clusters(self, sk, comp, kmer_size, cap=None):
        """rtc_upgma_clusters: one average-linkage dendrogram per component of the labelling comp[g] of sk's sketches (any
        labels; components are numbered by their smallest member) over the quantised rtc_linkage_distance of the exact keys.
        Returns (merges, first): UMERGE_DT records with a and b as genome indices, component after component, and first[c] where
        component c's records start.  cap: room for the records (None: n, which always suffices); too small raises
        RTC_ERR_OVERFLOW, the needed count in self.upgma_merges_needed."""
        n = sk.n
        lab = np.ascontiguousarray(np.asarray(comp).astype(np.int64).astype(np.uint32))
        if lab.shape != (n,):
            raise ValueError("comp must hold one label per sketch")
        room = max(n, 1) if cap is None else int(cap)
        out = np.zeros(max(room, 1), dtype=UMERGE_DT)
        first = np.zeros(n + 1, dtype=np.uint64)
        nm = C.c_uint64(0)
        st = self.lib.rtc_upgma_clusters(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), n, _np_ptr(lab), int(kmer_size),
                                         _np_ptr(out), room, C.byref(nm), _np_ptr(first))
        self.upgma_merges_needed = int(nm.value)
        self.check(st)
        return out[:nm.value].copy(), first[:len(np.unique(lab)) + 1].copy()

    def upgma_counters(self):
        """rtc_upgma_counters as a dict (the last upgma or upgma_clusters call), and "paths": rtc_upgma_last_path's bits."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_upgma_counters(self.h, a))
        names = ("components", "wave_components", "workgroup_components", "grid_components", "merges", "row_rescans", "fill_ns", "distance_ns",
                 "agglomerate_ns", "total_ns")
        out = {k: int(a[i]) for i, k in enumerate(names)}
        out["paths"] = self.upgma_last_path()
        return out

    def upgma_last_path(self):
        """rtc_upgma_last_path: UPGMA_PATH_WAVE | UPGMA_PATH_WORKGROUP | UPGMA_PATH_GRID of the last call"""
        return int(self.lib.rtc_upgma_last_path(self.h))

    def upgma_scan_blocks(self):
        """rtc_upgma_scan_blocks: RTC_UPGMA_SCAN_BLOCKS as the context holds it, 1 .. UPGMA_SCAN_BLOCKS (unset: UPGMA_SCAN_BLOCKS)"""
        return int(self.lib.rtc_upgma_scan_blocks(self.h))

    def graph_query(self, sk, n_db, threshold, kmer_size, knn_k=0, query_chunk=0, cap=None):
        """clust-leiden --db --assign, first call (rtc_graph_query): sk holds the n_db model genomes, then the queries.  Returns
        (edges, near): QEDGE_DT records (q, p, common) in (q, p) order -- every query's knn_k best model genomes among those
        passing graph_build's edge rule, knn_k 0: all of them -- and NEAR_DT per query.  cap: room for the records (None: the
        call is repeated with the count it reports); an explicit cap that is too small raises RTC_ERR_OVERFLOW, the needed
        count in self.graph_edges_needed."""
        nq = sk.n - int(n_db)
        if nq < 0:
            raise ValueError("n_db exceeds the sketch set")
        room = max(int(cap) if cap is not None else 64 * max(nq, 1), 1)
        near = np.zeros(max(nq, 1), dtype=NEAR_DT)
        while True:
            out = np.zeros(room, dtype=QEDGE_DT)
            ne = C.c_uint64(0)
            st = self.lib.rtc_graph_query(self.h, _t_ptr(sk.hashes), sk.width, _t_ptr(sk.start), _t_ptr(sk.len), int(n_db), nq,
                                          float(threshold), int(kmer_size), int(knn_k), int(query_chunk), _np_ptr(out),
                                          int(cap) if cap is not None else room, C.byref(ne), _np_ptr(near))
            self.graph_edges_needed = int(ne.value)
            if st == _lib.RTC_ERR_OVERFLOW and cap is None:
                room = int(ne.value)
                continue
            self.check(st)
            return out[:ne.value].copy(), near[:nq].copy()

    def graph_query_counters(self):
        """rtc_graph_query_counters as a dict (the last graph_query call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_graph_query_counters(self.h, a))
        names = ("chunks", "candidates", "passing", "kept", "queries_cut", "queries_alone", "join_ns", "filter_ns", "select_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}

    def leiden_place(self, labels, n_clusters, n_queries, edges, resolution=1.0, objective="cpm", tot=None, m2=0):
        """clust-leiden --db --assign, second call (rtc_leiden_place): labels are the model's (one per model genome, in
        [0, n_clusters)), edges WEDGE_DT records (u: query index, v: model genome, q) in any order.  objective "modularity"
        needs the model's tot (one per cluster) and m2; under "cpm" both are left out.  Returns PLACEMENT_DT per query: label
        (-1: novel), runner_up, n_edges, n_comms, k_x, e_label, e_runner."""
        obj = {"cpm": 0, "modularity": 1}.get(objective, objective)
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32))
        e = np.ascontiguousarray(np.asarray(edges, dtype=WEDGE_DT))
        t = None if tot is None else np.ascontiguousarray(np.asarray(tot, dtype=np.uint64))
        if t is not None and t.shape != (int(n_clusters),):
            raise ValueError("tot needs one entry per cluster")
        out = np.zeros(max(int(n_queries), 1), dtype=PLACEMENT_DT)
        self.check(self.lib.rtc_leiden_place(self.h, int(lab.size), _np_ptr(lab) if lab.size else None, int(n_clusters),
                                             _np_ptr(t) if t is not None and t.size else None, int(m2), float(resolution), int(obj),
                                             int(n_queries), _np_ptr(e) if e.size else None, int(e.size), _np_ptr(out)))
        return out[:int(n_queries)].copy()

    def leiden_place_counters(self):
        """rtc_leiden_place_counters as a dict (the last leiden_place call); row_paths: bit 0 one wave, bit 1 a 256-lane
        workgroup, bit 2 the global table (rtc_leiden_place_last_path)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_leiden_place_counters(self.h, a))
        names = ("records", "entries", "queries_with_records", "placed", "novel", "wave_rows", "workgroup_rows", "global_rows", "kernel_ns",
                 "total_ns")
        out = {k: int(a[i]) for i, k in enumerate(names)}
        out["row_paths"] = int(self.lib.rtc_leiden_place_last_path(self.h))
        return out

    def dbscan_counters(self):
        """rtc_dbscan_counters as a dict (the last dbscan call)."""
        a = (C.c_uint64 * 10)()
        self.check(self.lib.rtc_dbscan_counters(self.h, a))
        names = ("chunks", "candidate_edges", "eps_edges", "core_points", "asymmetric_pairs", "hook_rounds", "pair_ns",
                 "filter_ns", "components_ns", "total_ns")
        return {k: int(a[i]) for i, k in enumerate(names)}


def _hier_args(forest, core):
    forest = np.ascontiguousarray(forest, dtype=HEDGE_DT)
    core = np.ascontiguousarray(core, dtype=KDIST_DT)
    return forest, core, (forest if forest.size else np.zeros(1, dtype=HEDGE_DT)), (core if core.size else np.zeros(1, dtype=KDIST_DT))


def _hier_check(st, what):
    if st != _lib.RTC_OK:
        raise RtcError(st, what)


def hierarchy_cut(forest, core, eps_max, eps, kmer_size):
    """rtc_hierarchy_cut (host only): DBSCAN*'s clusters at eps <= eps_max from Context.dbscan_hierarchy's result.  Returns
    (int32 labels, bool core flags): clusters numbered by smallest core index, every non-core point -1 (no border attachment)."""
    forest, core, fb, cb = _hier_args(forest, core)
    n = int(core.size)
    labels, flags, ncl = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint8), C.c_uint32(0)
    _hier_check(_lib.load().rtc_hierarchy_cut(n, _np_ptr(fb), int(forest.size), _np_ptr(cb), float(eps_max), float(eps), int(kmer_size),
                                              _np_ptr(labels), _np_ptr(flags), C.byref(ncl)),
                "hierarchy_cut: eps %g (eps_max %g, k %d)" % (eps, eps_max, kmer_size))
    return labels[:n].copy(), flags[:n].astype(bool)


def hierarchy_flat(forest, core, kmer_size, min_cluster_size, return_stability=False):
    """rtc_hierarchy_flat (host only): the flat clustering of the condensed tree by excess of mass; int32 labels numbered by
    smallest member, -1 elsewhere.  return_stability: (labels, float64 stability per cluster)."""
    forest, core, fb, cb = _hier_args(forest, core)
    n = int(core.size)
    labels, stab, ncl = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.float64), C.c_uint32(0)
    _hier_check(_lib.load().rtc_hierarchy_flat(n, _np_ptr(fb), int(forest.size), _np_ptr(cb), int(kmer_size), int(min_cluster_size),
                                               _np_ptr(labels), _np_ptr(stab), C.byref(ncl)),
                "hierarchy_flat: min_cluster_size %d, k %d" % (min_cluster_size, kmer_size))
    return (labels[:n].copy(), stab[:ncl.value].copy()) if return_stability else labels[:n].copy()


def graph_weight(common, size_u, size_v, kmer_size):
    """rtc_graph_weight: 1 - calculate_mash_distance_fast (src/leiden.cpp:109-121), the library's host function"""
    return float(_lib.load().rtc_graph_weight(int(common), int(size_u), int(size_v), int(kmer_size)))


def _weight_units(edges, weights):
    """WEDGE_DT records: q = max(1, llround(weight * 2^20))"""
    out = np.zeros(len(edges), dtype=WEDGE_DT)
    out["u"], out["v"] = edges["u"], edges["v"]
    x = np.asarray(weights, dtype=np.float64) * 1048576.0
    low = np.floor(x)  # llround: x - floor(x) is exact, halves go away from zero
    out["q"] = np.maximum(1, low + (x - low >= 0.5)).astype(np.uint32)
    return out


def graph_weights(edges, sizes, kmer_size):
    """WEDGE_DT records of GEDGE_DT edges: q = max(1, llround(weight * 2^20)) of rtc_graph_weight"""
    fn = _lib.load().rtc_graph_weight
    return _weight_units(edges, [fn(c, sizes[u], sizes[v], kmer_size)
                                 for u, v, c in zip(edges["u"].tolist(), edges["v"].tolist(), edges["common"].tolist())])


def graph_denom(edges):
    """the truncated denom of graph_build_mash's edges (rtc_gedge.pad)"""
    return edges["pad"]


def graph_weight_mash(common, denom, sketch_size, kmer_size):
    """rtc_graph_weight_mash: 1 - rtc_mash_distance(common, denom), the library's host function"""
    return float(_lib.load().rtc_graph_weight_mash(int(common), int(denom), int(sketch_size), int(kmer_size)))


def graph_weights_mash(edges, sketch_size, kmer_size, return_weights=False):
    """WEDGE_DT records of graph_build_mash's edges: q = max(1, llround(w * 2^20)), w = rtc_graph_weight_mash(common, denom);
    return_weights: also the doubles w"""
    fn = _lib.load().rtc_graph_weight_mash
    w = np.array([fn(c, d, int(sketch_size), int(kmer_size)) for c, d in zip(edges["common"].tolist(), graph_denom(edges).tolist())],
                 dtype=np.float64)
    out = _weight_units(edges, w)
    return (out, w) if return_weights else out


def snn_weight(shared, deg_u, deg_v):
    """rtc_snn_weight: (shared + 2) / (deg_u + deg_v - shared), the library's host function"""
    return float(_lib.load().rtc_snn_weight(int(shared), int(deg_u), int(deg_v)))


def screen_identity(common, size, kmer_size):
    """rtc_screen_identity: Mash's containment identity (common / size) ** (1 / kmer_size), the library's host function"""
    return float(_lib.load().rtc_screen_identity(int(common), int(size), int(kmer_size)))


def linkage_distance(common, denom, kmer_size):
    """rtc_linkage_distance: the distance the host gives a complete-linkage merge of key common / denom"""
    return float(_lib.load().rtc_linkage_distance(int(common), int(denom), int(kmer_size)))


def jackknife_word(hash, seed, word):
    """rtc_jackknife_word: the 64 keep bits of a hash for the replicates 64 * word .. 64 * word + 63 (no GPU needed)"""
    return int(_lib.load().rtc_jackknife_word(int(hash) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF, int(word)))


def support_keep_table(kmer_size, threshold, max_denom):
    """rtc_support_keep_table: need[0 .. max_denom] as uint32 -- need[d] the least common count in 1 .. d whose distance at
    denominator d is at most the threshold, d + 1 where there is none (no GPU needed)"""
    out = np.zeros(int(max_denom) + 1, dtype=np.uint32)
    st = _lib.load().rtc_support_keep_table(int(kmer_size), float(threshold), int(max_denom), _np_ptr(out))
    if st != 0:
        raise _lib.RtcError(st, "rtc_support_keep_table(%r, %r, %r)" % (kmer_size, threshold, max_denom))
    return out


def upgma_distance(sum, size_a, size_b):
    """rtc_upgma_distance: the height of an average-linkage merge, sum / ((size_a size_b) 2^20) in double, through the library
    (no GPU needed)"""
    return float(_lib.load().rtc_upgma_distance(int(sum), int(size_a), int(size_b)))


def upgma_keep(sum, size_a, size_b, threshold):
    """clust-mst --upgma's cut rule in integers: a merge applies while sum <= qcut size_a size_b, qcut = llround(threshold 2^20)
    (round half away from zero, as the C library's llround)"""
    x = float(threshold) * 1048576.0
    lo = math.floor(abs(x))
    qcut = (int(lo) + (1 if abs(x) - lo >= 0.5 else 0)) * (1 if x >= 0 else -1)  # abs(x) - lo is exact
    return int(sum) <= qcut * int(size_a) * int(size_b)


def silhouette_value(records):
    """rtc_silhouette_value of every SIL_DT record, as a float64 array: (b - a) / max(a, b) with a = a_num / (a_den 2^20) and b
    likewise, each step one double operation; 0 where a_den or b_den is 0 or both means are."""
    r = np.atleast_1d(np.asarray(records, dtype=SIL_DT))
    ok = (r["a_den"] != 0) & (r["b_den"] != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = r["a_num"].astype(np.float64) / (r["a_den"].astype(np.float64) * 1048576.0)
        b = r["b_num"].astype(np.float64) / (r["b_den"].astype(np.float64) * 1048576.0)
        hi = np.maximum(a, b)
        v = (b - a) / hi
    return np.where(ok & (hi != 0.0), v, 0.0)


def silhouette_value_one(record):
    """rtc_silhouette_value of one SIL_DT record through the library (no GPU needed)"""
    r = np.ascontiguousarray(np.asarray(record, dtype=SIL_DT).reshape(1))
    return float(_lib.load().rtc_silhouette_value(_np_ptr(r)))


def linkage_bound(threshold, kmer_size):
    """the conservative stop bound (num, den) clust-mst --linkage complete passes: J = 1 / (2 exp(k d) - 1), times (1 - 2^-20),
    as floor(J 2^31) / 2^31"""
    j = 1.0 / (2.0 * np.exp(float(kmer_size) * float(threshold)) - 1.0) * (1.0 - 2.0 ** -20)
    return (int(np.floor(j * 2147483648.0)) if j > 0 else 0, 1 << 31)


def kdist_distance(common, size_p, size_q, kmer_size):
    """The distance of one rtc_kdist record: -ln(2 j / (1 + j)) / kmer_size with j = common / (size_p + size_q - common), in
    double with the C library's log; 0 where j = 1 (two empty u64 sketches included)."""
    denom = int(size_p) + int(size_q) - int(common)
    if denom == int(common):
        return 0.0
    j = float(common) / float(denom)
    return -math.log(2.0 * j / (1.0 + j)) / kmer_size


class Comm:
    """One rtc_comm (RCCL communicator of one GPU / context).  Ranks are processes (init_rank, the id
    from rank 0 travels through the launcher's channel, e.g. torch.distributed) or threads of one
    process (init_all)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        lib = ctx.lib
        self.rank, self.size = lib.rtc_comm_rank(handle), lib.rtc_comm_size(handle)
        self.backend = lib.rtc_comm_backend(handle).decode()

    @staticmethod
    def unique_id(lib=None):
        lib = lib or _lib.load()
        buf = (C.c_char * 128)()
        st = lib.rtc_comm_unique_id(buf)
        if st != _lib.RTC_OK:
            raise RtcError(st, "rtc_comm_unique_id: " + lib.rtc_last_error(None).decode(errors="replace"))
        return bytes(buf)

    @staticmethod
    def init_rank(ctx, nranks, rank, uid):
        h = C.c_void_p()
        buf = (C.c_char * 128).from_buffer_copy(uid) if uid is not None else None
        ctx.check(ctx.lib.rtc_comm_init_rank(ctx.h, nranks, rank, buf, C.byref(h)))
        return Comm(ctx, h)

    @staticmethod
    def init_all(ctxs):
        n = len(ctxs)
        hs = (C.c_void_p * n)(*[c.h for c in ctxs])
        out = (C.c_void_p * n)()
        st = ctxs[0].lib.rtc_comm_init_all(hs, n, out)
        ctxs[0].check(st)
        return [Comm(c, C.c_void_p(out[i])) for i, c in enumerate(ctxs)]

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.rtc_comm_destroy(self.h)
            self.h = None

    def all_reduce(self, t, op="min"):
        dtype = {torch.int64: 0, torch.int32: 1}[t.dtype]
        self.ctx.check(self.ctx.lib.rtc_comm_all_reduce(self.h, _t_ptr(t), t.numel(), dtype, 0 if op == "min" else 1))

    def all_reduce_host(self, vals, op="max"):
        a = np.ascontiguousarray(vals, dtype=np.int64)
        self.ctx.check(self.ctx.lib.rtc_comm_all_reduce_host(self.h, _np_ptr(a), len(a), 0 if op == "min" else 1))
        return a

    def gather_rows(self, t_global, n_local, a, b, async_=False):
        row_bytes = t_global.numel() * t_global.element_size() // (self.size * n_local)
        self.ctx.check(self.ctx.lib.rtc_comm_gather_rows(self.h, _t_ptr(t_global), row_bytes, n_local, a, b, int(async_)))

    def wait(self):
        self.ctx.check(self.ctx.lib.rtc_comm_wait(self.h))


# ---- host-side arithmetic shared by CLI-equivalent flows (reference expression order) -------------
RADIO_MAX = 0x7FFFFFFF


def mst_radio(threshold, kmer_size):
    """src/MST.cpp:26-37,1292: floor(2*exp(thr*(k-1)) - 1), saturated at INT32_MAX (rtc_size_radio in csrc/rtc_internal.h):
    the value crosses the C ABI as an int, and a saturated radio keeps every pair."""
    try:
        r = 2.0 * math.exp(threshold * (kmer_size - 1)) - 1.0
    except OverflowError:  # where C's exp gives +inf
        return RADIO_MAX
    return int(r) if r < RADIO_MAX else RADIO_MAX


def mst_distance(common, size0, size1, kmer_size, is_containment):
    """src/MST.cpp:1295,1489-1515 evaluated with the same operation order (host libm)."""
    inv_k = 1.0 / kmer_size
    if not is_containment:
        denom = size0 + size1 - common
        jac = 0.0 if denom == 0 else common / denom
        if jac == 1.0:
            return 0.0
        if jac == 0.0:
            return 1.0
        ratio = (2.0 * jac) / (1.0 + jac)
        return -inv_k * math.log(ratio)
    denom = min(size0, size1)
    c = 0.0 if denom == 0 else common / denom
    if c == 1.0:
        return 0.0
    if c == 0.0:
        return 1.0
    return -inv_k * math.log(c)


class PackedBatch:
    """A batch in the command lines' 2-bit staging format, resident in HBM (include/rtclust.h, rtc_unpack_bases_dev):
    `packed` uint8[n_bases / 4], `runs` int64[2 r] = (start, length) of every stretch outside ACGT (ascending)."""

    def __init__(self, packed, n_bases, runs):
        self.packed, self.n_bases, self.runs = packed, int(n_bases), runs


def pack_staging(seq, total):
    """Characters resident in HBM -> PackedBatch, what the command lines' parser produces on the host (rtc_host.cpp:
    PackedSink).  Torch plumbing for benchmarks and tests, in pieces that keep the temporaries small; not a product path."""
    total = int(total)
    n_bases = (total + 63) // 64 * 64 + 64
    dev = seq.device
    packed = torch.empty(n_bases // 4, dtype=torch.uint8, device=dev)
    runs = []
    step = 1 << 28
    for a in range(0, n_bases, step):
        b = min(a + step, n_bases)
        x = seq[a:min(b, total)]
        if x.numel() < b - a:
            x = torch.cat([x, torch.full((b - a - x.numel(),), ord("N"), dtype=torch.uint8, device=dev)])
        c = (((x >> 1) ^ (x >> 2)) & 3).view(-1, 4)
        packed[a // 4:b // 4] = c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)
        up = x & 0xDF
        idx = torch.nonzero(~((up == 65) | (up == 67) | (up == 71) | (up == 84))).view(-1)
        if idx.numel():
            first = torch.ones_like(idx, dtype=torch.bool)
            first[1:] = idx[1:] != idx[:-1] + 1
            last = torch.ones_like(idx, dtype=torch.bool)
            last[:-1] = first[1:]
            starts, ends = idx[first], idx[last] + 1
            runs.append(torch.stack([starts + a, ends - starts], dim=1).reshape(-1))  # a stretch across a seam: two runs that touch
        del x, c, up, idx
    runs = torch.cat(runs).contiguous() if runs else torch.zeros(0, dtype=torch.int64, device=dev)
    return PackedBatch(packed, n_bases, runs)


def synth_family_descs(n_families, per_family, global_seed=42, max_rate=0.08, n_every=0):
    """SURVEY.md 8d synthetic design: families of `per_family` members, member 0 is the ancestor,
    member m>0 carries substitutions at rate U[0,max_rate] drawn from a counter-based stream."""
    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)
    n = n_families * per_family
    d = np.zeros(n, dtype=SYNTH_DT)
    for f in range(n_families):
        fs = mix((global_seed << 20) ^ (f * 2 + 1))
        for m in range(per_family):
            g = f * per_family + m
            ms = mix(fs ^ (m * 0x632BE59BD9B4E019 & 0xFFFFFFFFFFFFFFFF))
            rate = 0.0 if m == 0 else max_rate * ((mix(ms ^ 0xABCDEF) >> 11) / float(1 << 53))
            d[g] = (fs, ms, int(rate * 16384), n_every)
    return d
