"""`Tracker`: drop-in for `pymht.tracker.Tracker`, running on one MI355X.

Same constructor, `preInitialize`, `initiateTarget`, `addMeasurementList(scanList, aisList=AisMessageList(), **kw)`,
`getTrackNodes`, `getRuntimeAverage`, `runtimeLog`/`toc` keys and double-underscore attributes as the reference
(pymht/tracker.py:39-307).  Steps 1-6 of a scan (grow, cluster, optimise, terminate, N-scan
prune) run as two HIP launches (grow incl. the clustering's union-find, ILP; the report rides in the next scan's grow launch) on the
device-resident hypothesis forest of libmht_amd.so (include/mht_amd.h); the host sees one report per scan.  Step 7 (M-of-N initiation) runs on the device as well (`useInitiator`).

XML result export: `getScenarioElement` / `_storeTrackerArgs` / `_storeRun` (tracker.py:1469-1545).
AIS-aided tracking (tracker.py:394-396, :417-552; tracks started from AIS messages m_of_n.py:262-280): construct with
`aisAided=True` (and a finite `radarRange`), then `addMeasurementList(scan, aisList)`.  Not supported (raise): `dynamicWindow`.
There is no CPU fallback: without the HIP library or without a GPU the constructor raises.
"""
import ctypes as C
import logging
import os
import time

import numpy as np

from . import _lib
from .device import Context, make_model
from .initiators import m_of_n
from .models import pv
from .pyTarget import Target
from .utils.classDefinitions import AisMessageList, MeasurementList  # noqa: F401
from .utils import xmlDefinitions as xmltags
from .utils.xmlDefinitions import activeTag, outofrangeTag, preinitializedTag, toolowscoreTag

log = logging.getLogger(__name__)

def _report_dtypes(nx):
    """NumPy views of mht_target_report / mht_birth_report for the nx-state build of the library (include/mht_amd.h: MHT_NX)."""
    rep = np.dtype([("id", "<i4"), ("status", "<i4"), ("sel_node", "<i4"), ("sel_meas", "<i4"),
                    ("new_index", "<i4"), ("root_scan", "<i4"), ("root_node", "<i4"), ("n_leaves", "<i4"),
                    ("sel_x", "<f8", (nx,)), ("sel_cnllr", "<f8"), ("score", "<f8"), ("root_cnllr", "<f8"),
                    ("root_x", "<f8", (nx,)), ("root_meas", "<i4"), ("cluster", "<i4")])
    birth = np.dtype([("id", "<i4"), ("meas", "<i4"), ("x0", "<f8", (nx,)), ("P0", "<f4", (nx * nx,))])
    return rep, birth


_REPORT_DTYPE, _BIRTH_DTYPE = _report_dtypes(4)
assert _REPORT_DTYPE.itemsize == C.sizeof(_lib.MhtTargetReport) and _BIRTH_DTYPE.itemsize == C.sizeof(_lib.MhtBirthReport)
assert _report_dtypes(6)[0].itemsize == C.sizeof(_lib.MhtTargetReport6) and _report_dtypes(6)[1].itemsize == C.sizeof(_lib.MhtBirthReport6)
_F_COV_F64 = 16      # include/mht_amd.h: MHT_F_COV_F64
_STATUS_TAG = {0: activeTag, 1: outofrangeTag, 2: toolowscoreTag, 3: toolowscoreTag}


class DeviceTarget(Target):
    """A `Target` that mirrors one node of the device forest (`scanNumber`, `_node` locate it)."""
    _tracker = None
    _node = -1
    _hist_mmsi = None      # AIS forest: the identity the node's track is bound to, as the device keeps it per node
    _P_lazy = False        # the covariance handed to the constructor is a placeholder: the node's own is fetched from the device when somebody reads it
    _P = None

    @property
    def P_0(self):
        if self._P_lazy:
            self._P_lazy = False
            t = self._tracker
            # (the constructor's placeholder is the tracker-wide default P_0, not this node's covariance: a node the device cannot answer for
            # any more -- it has left the ring, or reports are still pending -- has NO covariance to show, not a wrong one)
            self._P = None
            if t is not None and self._node >= 0 and self.scanNumber is not None and 0 <= len(t.__scanHistory__) - self.scanNumber < t._cfg.n_scan + 4:
                try:
                    P = t._window_chain(self.scanNumber, self._node)[4]
                    if len(P):
                        self._P = np.array(P[0]).reshape(t.nx, t.nx)
                except _lib.MhtError:
                    pass      # (the node has left the device ring)
        return self._P

    @P_0.setter
    def P_0(self, value):
        self._P, self._P_lazy = value, False

    def _getHistoricalMmsi(self):
        """pyTarget.py:297-302; the device carries the answer with every node (own identity, else the nearest AIS-updated ancestor's)."""
        if self._hist_mmsi is not None:
            return self._hist_mmsi
        return Target._getHistoricalMmsi(self)

    def getLeafNodes(self):
        if self._children is None and self.isRoot and self._tracker is not None:
            return self._tracker._leaf_views(self)
        return Target.getLeafNodes(self)


class Tracker():

    def __init__(self, model, radarPeriod, lambda_phi, lambda_nu, **kwargs):
        # Radar parameters (tracker.py:43-51)
        self.position = kwargs.get('position', np.array([0., 0.]))
        self.radarRange = kwargs.get('radarRange', float('inf'))
        self.radarPeriod = radarPeriod
        self.fixedPeriod = True
        self.default_P_d = kwargs.get('P_d', 0.8)
        assert self.default_P_d < 1 and self.default_P_d > 0, "Invalid P_d"
        # State space model (tracker.py:53-59)
        self.A = model.Phi(radarPeriod)
        self.C = model.C_RADAR
        self.P_0 = model.P0
        self.R_RADAR = model.R_RADAR()
        self.Q = model.Q(radarPeriod)
        # Target initiator (tracker.py:61-72)
        self.maxSpeedMS = kwargs.get('maxSpeedMS', 20)
        self.M_required = kwargs.get('M_required', 2)
        self.N_checks = kwargs.get('N_checks', 3)
        self.mergeThreshold = 4 * (model.sigmaR_RADAR_tracker ** 2)
        # Tracker storage (tracker.py:74-84): the forest lives on the device; the host keeps flat NumPy tables and
        # builds `Target` views only when somebody looks (properties __targetList__, __trackNodes__, ... below)
        self.__scanHistory__ = []
        self._scan_times = np.zeros(256)     # time of scan k at index k (index 0 = before the first scan); grows by doubling
        self.__aisHistory__ = []
        self.trackIdCounter = 0
        # Timing and logging (tracker.py:86-101)
        self._runtimeLog_ = {k: [] for k in ('Total', 'Process', 'Cluster', 'Optim', 'ILP-Prune', 'DynN', 'N-Prune',
                                           'Terminate', 'Init')}
        self.tic = {}
        self._toc_ = {}
        self._nOptimSolved_ = 0
        # Tracker parameters (tracker.py:103-118)
        self.pruneSimilar = kwargs.get('pruneSimilar', False)
        self.lambda_phi = lambda_phi
        self.lambda_nu = lambda_nu
        self.lambda_ex = lambda_phi + lambda_nu
        self.eta2 = kwargs.get('eta2', 5.99)
        self.eta2_ais = kwargs.get('eta2_ais', 9.45)
        N = kwargs.get('N', 5)
        self.N_max = N
        self.N = N
        self.scoreUpperLimit = -np.log(1 - self.default_P_d) * 0.8
        self.clnnrUpperLimit = 3.0
        self.pruneThreshold = kwargs.get("pruneThreshold", 4)
        self.targetSizeLimit = 3000      # (tracker.py:118: only used by the reference's dynamic window; kept for the XML settings block)
        self._prune_similar_on = False      # (what the device forest is currently set to; decided per scan like the reference does)
        # MI355X side
        # state dimension: 4 (the reference's models/pv) or 6 (e.g. pymht_amd.models.ca -- BASELINE config 5 names a six-state model; the
        # reference's kalman module is dimension-generic, its tracker and initiator are not): the six-state build of the library
        self.nx = int(np.asarray(self.C).shape[1])
        assert self.nx in (4, 6), "pymht_amd is built for 4- and 6-state models"
        self._REPORT_DTYPE, self._BIRTH_DTYPE = _report_dtypes(self.nx)
        self.useInitiator = kwargs.get('useInitiator', self.nx == 4)
        # six-state model: the 4-state initiator's births enter the forest lifted, x = [x4, t], P = [[P4, 0], [0, Pt]] (mht_initiator_set_lift);
        # (t, Pt) = birthTail, by default zeros and the model's own P0[4:, 4:]
        self.liftBirths = bool(kwargs.get('liftBirths', False))
        if self.useInitiator and self.nx != 4 and not self.liftBirths:
            raise NotImplementedError("the M-of-N initiator is the reference's 4-state one (m_of_n.py imports models/pv): useInitiator=False for a "
                                      "six-state model, or liftBirths=True to start its births as [x, y, vx, vy] + birthTail (default: zeros, model.P0[4:, 4:])")
        birth_tail = kwargs.get('birthTail', None)
        if birth_tail is None:
            birth_tail = (np.zeros(self.nx - 4), np.asarray(model.P0)[4:, 4:])
        self._birth_tail = (np.asarray(birth_tail[0], np.float32).reshape(self.nx - 4), np.asarray(birth_tail[1], np.float32).reshape(self.nx - 4, self.nx - 4))
        self._ctx = Context(kwargs.get('device', 0), nx=self.nx)
        self._lib = self._ctx.lib
        self._model = make_model(self.A, self.Q, self.C, self.R_RADAR, self.eta2, self.lambda_ex, self.default_P_d)
        cfg = _lib.MhtForestConfig()
        cfg.max_targets = int(kwargs.get('maxTargets', 2048))
        cfg.max_nodes = int(kwargs.get('maxNodes', 1 << 19))
        cfg.max_meas = int(kwargs.get('maxMeasurements', 2048))
        cfg.n_scan = int(N)
        cfg.blp_max_iter = int(kwargs.get('blpMaxIter', 200))
        cfg.blp_node_limit = int(kwargs.get('blpNodeLimit', 1 << 20))
        self._blp_time_limit = kwargs.get('blpTimeLimit', None)      # seconds of branch and bound per cluster (None: exact, however long)
        cfg.score_limit = float(self.scoreUpperLimit)
        cfg.cnllr_limit = float(self.clnnrUpperLimit)
        cfg.radar_x, cfg.radar_y = float(self.position[0]), float(self.position[1])
        cfg.radar_range = float(self.radarRange)
        cfg.merge_threshold = float(self.mergeThreshold)
        self._cfg = cfg
        # AIS-aided tracking (tracker.py:394-396, :417-552): the forest has to be made for it (identities per node, AIS rows in the ILP);
        # `aisAided=True` is the switch -- the reference decides per call by looking at its aisList, a device forest cannot
        self._ais = bool(kwargs.get('aisAided', False))
        self._model_mod = model
        self.P_ais = 0.5                                    # tracker.py:109
        self._leaf_time = None                              # time of the current leaves (the last scan's, or the initial targets')
        if self._ais:
            if self.nx != 4:
                raise NotImplementedError("AIS messages report four states (models/ais.py): aisAided needs a 4-state model")
            _lib.check(self._lib.mht_forest_create_ex(self._ctx.handle, C.byref(self._model), C.byref(cfg), 1))      # MHT_FOREST_AIS
        elif getattr(model, "transition", None) == "ct":
            # a state-dependent transition (pymht_amd/models/ct.py, BASELINE config 5's constant-turn model): Phi(T, w) per hypothesis, the
            # reference's per-hypothesis form kalman.predict_single + kalman.precalc (kalman.py:67-70, :82-101); self.A = Phi(T, 0) carries T
            if self.nx != 6:
                raise NotImplementedError("the constant-turn model has six states")
            _lib.check(self._lib.mht_forest_create_ex(self._ctx.handle, C.byref(self._model), C.byref(cfg), 2))      # MHT_FOREST_CT
        else:
            _lib.check(self._lib.mht_forest_create(self._ctx.handle, C.byref(self._model), C.byref(cfg)))
        if self._blp_time_limit is not None:
            _lib.check(self._lib.mht_forest_set_blp_time_limit(self._ctx.handle, 1e3 * float(self._blp_time_limit)))
        # Target initiator (tracker.py:61-72): on the device, behind every scan's commit (mht_forest_initiate).  It is the reference's 4-state one
        # whatever the model: a six-state tracker hands it models/pv's measurement matrices, and the forest lifts its births
        init_C, init_R = (self.C, self.R_RADAR) if self.nx == 4 else (pv.C_RADAR, pv.R_RADAR())
        self.initiator = m_of_n.Initiator(self.M_required, self.N_checks, self.maxSpeedMS, init_C, init_R, self.mergeThreshold,
                                          ctx=self._ctx, maxMeasurements=cfg.max_meas, default_pd=self.default_P_d) \
            if self.useInitiator else None
        if self.initiator is not None and self.nx != 4:
            self.initiator.set_lift(self.nx, *self._birth_tail)
        # per-stage device times (toc['Process'], ['Cluster'], ['Optim'], ['N-Prune']: five HIP events per scan and a stream
        # synchronisation to read them): off by default, it keeps the host from running ahead of the device
        self._timing = bool(kwargs.get('deviceTiming', False))
        _lib.check(self._lib.mht_forest_set_timing(self._ctx.handle, int(self._timing)))
        # host mirror of the target list (one row per target, target-list order)
        self._tbl_ = np.zeros(0, dtype=self._REPORT_DTYPE)      # (only id, root_scan, root_node, root_meas, root_x, root_cnllr are read)
        self._sel_ = None            # report records of the live targets after the last scan (selected leaves)
        self._labels = np.zeros(0, np.int64)
        self._labels_src = None      # the report rows of the last scan: their `cluster` column is read when somebody asks for the clusters
        self._history = []          # chunks of committed roots: dict(id, scan, node, meas, x, cnllr, time) arrays
        self._history_mmsi = []     # AIS forest: the identities of those roots, chunk by chunk (0 = none)
        self._last_ais_scan = -(1 << 30)      # last scan that carried AIS messages
        self._dead_chunks = []      # [records, scan time, scan number, z, window chains or None, ticket, fold number] of terminated tracks
        self._chain_pending = []    # the entries of _dead_chunks whose chains are still on their way (mht_forest_chains_begin)
        self._fold_no = 0
        self._birth = {}            # Target.ID -> (time, scan, x, P, meas, measurement, status)
        self._views = {}            # cache of lazily built views, dropped at every scan
        self._scanStatsLog = [] if kwargs.get('logScanStats', False) else None      # lastScanStats (+ nTargets) of every scan (property scanStatsLog)
        self._pendq = []            # the scans whose reports are still on their way, oldest first (folded by later scans or by the first look)
        self._dead = False          # a device step failed: the forest cannot go on
        self._staged = self._staged_prev = self._staged_np = None
        self._stats_ = {}
        self._scanrecs = []          # per-scan numbers of the folded reports that `toc` / `runtimeLog` / `lastScanStats` have not been built from yet
        self._rep = _lib.MhtScanReport(); self._rep_ref = C.byref(self._rep)
        self._rec_size = self._REPORT_DTYPE.itemsize
        self._no_recs = np.zeros(0, dtype=self._REPORT_DTYPE)

    # ------------------------------------------------------------------------------------------------
    def preInitialize(self, simList):
        """tracker.py:139-145: one root per ground-truth object of simList[0]."""
        # one batch: the device admits the candidates sequentially (each is tested against the leaves and against the
        # candidates admitted before it), exactly like calling initiateTarget one by one
        self._add_targets([Target(initialTarget.time, None, initialTarget.cartesianState(), self.P_0, status=preinitializedTag)
                           for initialTarget in simList[0]])

    def initiateTarget(self, newTarget):
        """tracker.py:147-160.  The neighbour test (pyTarget.py:181-189) runs on the device against the current
        leaves."""
        self._add_targets([newTarget])

    def _add_targets(self, targets):
        self._drain()
        n = len(targets)
        if n == 0:
            return []
        if self._ais:
            # the AIS-aided update steps every leaf from ITS time to the message's (tracker.py:448: node.time); the device keeps one time for
            # all leaves (the last scan's, or the initial targets'): a target of another time would get a wrong first time step
            lt = self._leaf_time if self._leaf_time is not None else float(targets[0].time)
            if any(float(t.time) != lt for t in targets):
                raise ValueError("aisAided tracker: an initiated target's time differs from the time of the current leaves (%r): "
                                 "the AIS time steps are built from one leaf time" % lt)
        x0 = np.ascontiguousarray(np.array([np.asarray(t.x_0, dtype=np.float64) for t in targets]).reshape(n, self.nx))
        P0 = np.ascontiguousarray(np.array([np.asarray(t.P_0, dtype=np.float32) for t in targets]).reshape(n, self.nx * self.nx))
        f32 = np.array([np.asarray(t.x_0).dtype == np.float32 for t in targets])
        flags = np.where(f32, _lib.F_STATE_F32 | _lib.F_SCORE_F32, 0).astype(np.uint8)
        pd = np.full(n, self.default_P_d, dtype=np.float64)
        meas = np.array([0 if t.measurementNumber is None else int(t.measurementNumber) for t in targets], dtype=np.int32)
        acc = np.zeros(n, dtype=np.uint8)
        ids = np.zeros(n, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.mht_forest_add_targets(self._ctx.handle, n, p(x0), p(P0), p(flags), p(pd), p(meas), 1,
                                                    p(acc), p(ids)))
        scan = len(self.__scanHistory__)
        ok = acc.astype(bool)
        out = [t for t, a in zip(targets, ok) if a]
        if not out:
            return out
        rows = np.zeros(len(out), dtype=self._REPORT_DTYPE)
        rows["id"], rows["root_scan"], rows["root_node"], rows["root_meas"], rows["root_x"] = ids[ok], scan, -1, meas[ok], x0[ok]
        self._tbl_ = np.concatenate([self._tbl_, rows])
        for t, i in zip(out, ids[ok]):
            self._birth[int(i)] = (t.time, scan, t.x_0, t.P_0, t.measurementNumber, t.measurement, t.status)
            t.ID = int(i)
        if scan == 0 and self._leaf_time is None:
            self._leaf_time = float(out[0].time)
        self.trackIdCounter = int(ids[ok].max()) + 1
        self._views.clear()
        return out

    # ------------------------------------------------------------------------------------------------
    def addMeasurementList(self, scanList, aisList=AisMessageList(), **kwargs):
        """tracker.py:162-307 for the radar-only case.

        Returns as soon as the scan is queued on the device: steps 1-7 run there without a host round trip, and the scan's report
        travels to pinned host memory behind them.  It is folded into the host mirror by the next call or by the first look at
        the tracker's state (every attribute / method that exposes results waits for it), so a host that streams scans in
        overlaps its own bookkeeping with the device's work."""
        tic = {'Total': time.time(), '_call': time.perf_counter()}
        z = self._accept_scan(scanList, aisList, kwargs)
        tic['_print'] = {k: v for k, v in kwargs.items() if k in ("printTime", "printCluster", "printInfo", "on_color") and v}
        self._set_prune_similar(bool(kwargs.get('pruneSimilar', False)))      # tracker.py:230: a per-scan switch (the constructor's copy is never read)
        if aisList is not None and len(aisList) > 0:
            self._arm_ais(scanList, aisList, z.shape[0], bool(kwargs.get('aisInitialization', True)))
            self._last_ais_scan = len(self.__scanHistory__) + len(self._pendq) + 1
        # The host mirror is only touched once the device has accepted the scan: a rejected step (too many measurements, dead
        # forest) leaves the tracker exactly as it was.
        try:
            self._staged, self._staged_np = None, z      # (the library stages the scan in pinned memory and copies it itself)
            _lib.check(self._lib.mht_forest_scan(self._ctx.handle, self.initiator.handle if self.useInitiator else None,
                                                 z.__array_interface__['data'][0], z.shape[0], float(scanList.time)))
        except _lib.MhtError as e:
            if e.code != _lib.MHT_E_INVALID:
                self._dead = True
            elif self._ais and self.useInitiator:      # (a refused scan must not leave its messages with the initiator for the next one)
                self._lib.mht_initiator_set_ais(self.initiator.handle, None, 0, None)
            raise
        tic['_call'] = time.perf_counter() - tic['_call']      # host time of this call up to here (the scan is queued; nothing waited)
        self._leaf_time = float(scanList.time)
        self._queue_report(scanList, z, aisList, tic)

    def _arm_ais(self, scanList, aisList, nRadarMeas, ais_init):
        """The AIS messages of this scan, handed to the device in the order the reference walks them (pymht_amd/ais.py).  Needs the
        folded state of the scan before (lambda_ais counts the targets, tracker.py:438), so a scan with messages does not overlap
        with its predecessor's report."""
        from .ais import group_messages, initiator_messages
        self._drain()
        scanTime = float(scanList.time)
        assert all(float(m.time) < scanTime for m in aisList)                                   # tracker.py:180-182
        assert all(float(m.time) > scanTime - self.radarPeriod for m in aisList), str(scanTime) + str([m.time for m in aisList])
        mmsi = [m.mmsi for m in aisList]
        assert len(mmsi) == len(set(mmsi)), "Duplicate MMSI in aisList"                          # tracker.py:183-185
        if not np.isfinite(self.radarRange):
            raise ValueError("AIS-aided tracking needs a finite radarRange (lambda_ais = nTargets * P_ais / (pi * radarRange^2), tracker.py:438; "
                             "with the default inf the reference itself fails in kalman.nllr)")
        if ais_init and self.useInitiator:      # the messages no track takes start preliminary tracks (tracker.py:267-273, m_of_n.py:262-280)
            msgs_i = initiator_messages(aisList, scanTime)
            _lib.check(self._lib.mht_initiator_set_ais(self.initiator.handle, C.byref(msgs_i), len(aisList), None))
        nT = len(self._tbl_)
        if nT == 0 or self._leaf_time is None:
            return                                                                               # (no leaves: nothing to fuse)
        lambda_ais = (nT * self.P_ais) / (np.pi * self.radarRange ** 2)
        groups, nG, msgs, order = group_messages(aisList, self._leaf_time, scanTime, self._model_mod)
        _lib.check(self._lib.mht_forest_set_ais(self._ctx.handle, C.byref(groups), nG, C.byref(msgs), len(order), float(self.eta2_ais), float(lambda_ais)))

    def _set_prune_similar(self, want):
        if want != self._prune_similar_on:
            _lib.check(self._lib.mht_forest_set_prune_similar(self._ctx.handle, float(self.pruneThreshold) if want else 0.0))
            self._prune_similar_on = want

    def _after_step(self, scanList, z, aisList, tic=None):
        """Behind the device step: step 7 on the device, then the report starts its way to the host."""
        if self.useInitiator:
            # 7 -- Initiate new tracks (tracker.py:264-278): on the device, right behind the scan's commit; what it gave birth to
            # comes back with the scan's report
            _lib.check(self._lib.mht_forest_initiate(self._ctx.handle, self.initiator.handle,
                                                     self._staged.data_ptr() if self._staged is not None else None, z.shape[0],
                                                     float(scanList.time)))
        _lib.check(self._lib.mht_forest_report_begin(self._ctx.handle))
        self._queue_report(scanList, z, aisList, tic)

    def _queue_report(self, scanList, z, aisList, tic):
        self._pendq.append((scanList, z, aisList, tic if tic is not None else {'Total': time.time()}))
        # With the device initiator the report of scan k leaves the device inside the grow launch of scan k + 1 (queued by the NEXT
        # call): folding it in that next call would wait for that launch -- report -> fold -> queue -> launch -> report is a latency
        # loop through the host, 85 us per scan whatever the device needs.  The call for scan k + 2 folds it instead, behind its own
        # queueing: it arrived a scan ago and nobody waits.  (Without the initiator the report travels right behind its own scan.)
        lag = 2 if (self.useInitiator and not self._timing) else 1
        if len(self._pendq) > lag:
            prev = self._pendq.pop(0)
            self._finish_scan(*prev, which=len(self._pendq))
        if self._timing:          # (the stage times are read scan by scan)
            self._drain()

    def _drain(self):
        """Fold the reports of the scans that are still in flight, oldest first (waits for them)."""
        if len(self._pendq) > 1:      # (the last scan's report would only start its way to the host when it is asked for: start it now, fold the older one meanwhile)
            _lib.check(self._lib.mht_forest_report_begin(self._ctx.handle))
        while self._pendq:
            prev = self._pendq.pop(0)
            self._finish_scan(*prev, which=len(self._pendq))

    def _accept_scan(self, scanList, aisList, kwargs):
        """Argument checks of addMeasurementList; returns the scan as the (M,2) float32 array the device gates."""
        if self._dead:
            raise RuntimeError("this Tracker's device forest is dead (an earlier scan failed); create a new Tracker")
        if aisList is not None and len(aisList) > 0:
            if not self._ais:
                raise NotImplementedError("this Tracker was not made for AIS messages: pass aisAided=True to the constructor (tracker.py:417-552)")
            if kwargs.get('aisInitialization', True) and not self.useInitiator:
                pass      # (no initiator: nothing starts tracks, like a reference tracker whose initiator was taken out)
        if kwargs.get('dynamicWindow', False):
            raise NotImplementedError("dynamicWindow is not supported by pymht_amd")
        m = np.asarray(scanList.measurements)
        z = np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 2)
        if m.dtype != np.float32 and m.size and not np.array_equal(z.astype(np.float64).reshape(m.shape), m.astype(np.float64)):
            # the reference gates in the dtype it is given (its simulator produces float32); the device takes float32
            log.warning("addMeasurementList: measurements are %s and not exactly representable as float32; they are rounded "
                        "(the reference would gate them in %s)", m.dtype, m.dtype)
        return z

    def _upload_scan(self, z):
        """The scan in device memory (a torch tensor of the tracker, kept alive until the scan after the next): device pointer."""
        import torch
        self._staged_np = z
        t = torch.from_numpy(z if z.size else np.zeros((1, 2), np.float32)).to(self._ctx.device, non_blocking=True)
        self._staged_prev, self._staged = self._staged, t
        return t.data_ptr()

    def _stage_scan(self, scanList, aisList=None, **kwargs):
        """SectorGroup: checks + the scan in device memory (a torch tensor kept alive until the next scan)."""
        z = self._accept_scan(scanList, aisList, kwargs)
        self._set_prune_similar(bool(kwargs.get('pruneSimilar', False)))
        self._upload_scan(z)
        return self._staged[:z.shape[0]] if z.size else self._staged[:0]

    def _finish_scan(self, scanList, z, aisList, tic, which=0):
        """The host side of a scan: wait for its report, fold it (and the device initiator's births) into the host mirror.

        Only what later scans need is done here -- the report's rows become the table of the live targets, births and terminated tracks
        are taken in -- and the scan's numbers are kept as one tuple; the dictionaries the reference exposes (`toc`, `runtimeLog`,
        `lastScanStats`, the scan log) are built from those tuples when somebody reads them (`_materialise`): a host that streams scans
        in pays a few microseconds per scan here, not thirty."""
        t_fold = time.perf_counter()
        t_init = time.time()
        self._fold_no += 1
        if self._chain_pending:      # (chains begun two folds ago were gathered in front of the scan this fold's report belongs to)
            self._resolve_chains(self._fold_no - 2)
        rep = self._rep
        rc = self._lib.mht_forest_report_get(self._ctx.handle, which, self._rep_ref)
        if rc == _lib.MHT_E_LIMIT:
            # soft: an ILP ran into the branch-and-bound node limit.  The selection it returned is feasible (not proven optimal)
            # and the device forest HAS advanced with it: fold the report like any other (the reference logs "Optim result NOT
            # optimal", tracker.py:1201, and carries on as well)
            log.warning("scan %d: %d ILP(s) hit the branch-and-bound node limit; their selection is feasible, not proven optimal",
                        rep.scan, rep.n_limit)
        elif rc:
            self._dead = True
            _lib.check(rc)
        hist = self.__scanHistory__
        hist.append(scanList)
        scanNumber = len(hist)
        if scanNumber >= len(self._scan_times):
            self._scan_times = np.concatenate([self._scan_times, np.zeros(len(self._scan_times))])
        scanTime = scanList.time
        self._scan_times[scanNumber] = scanTime
        self.__aisHistory__.append(aisList)
        nRadarMeas = z.shape[0]
        assert rep.scan == scanNumber
        nT = rep.n_targets
        # (one memcpy of the rows out of the pinned block, viewed as records: NumPy copies a structured array field by field, 12x slower)
        recs = np.frombuffer(C.string_at(rep.targets, nT * self._rec_size), dtype=self._REPORT_DTYPE) if nT else self._no_recs
        used_raw = C.string_at(rep.used, 8 * max(rep.used_words, 1))
        self._apply_report(recs, scanTime, scanNumber, z, rep.n_alive == nT)
        if rep.n_births:
            births = np.frombuffer(C.string_at(rep.births, rep.n_births * self._BIRTH_DTYPE.itemsize), dtype=self._BIRTH_DTYPE)
            self._apply_births(births, scanTime, scanNumber, z[self._unused_of(used_raw, nRadarMeas)])
        # toc['Total'] = what THIS scan cost: the host time of its addMeasurementList call + the device time of its stages + the host
        # time of folding its report.  NOT the wall time between the call and the fold: the report of scan k is folded by the call for
        # scan k+1 (or by the first look at the results), so that interval is the host's idle time between scans -- a real-time host
        # feeding one scan per radarPeriod would see Total ~ radarPeriod and a spurious "Did not pass real time demand".
        call = tic.get('_call', 0.0)
        stage = None
        if self._timing:
            ms = (C.c_float * 5)()
            _lib.check(self._lib.mht_forest_stage_times(self._ctx.handle, C.byref(ms), None))
            stage = (ms[0] * 1e-3, ms[1] * 1e-3, ms[2] * 1e-3, ms[3] * 1e-3, ms[4] * 1e-3)
        device = stage[4] if stage is not None else rep.t_scan * 1e-8
        now = time.perf_counter()
        total = call + device + (now - t_fold)
        # (rep is reused by the next fold: the numbers are taken out now)
        self._scanrecs.append((tic, rep.t_process, rep.t_cluster, rep.t_optim, rep.t_scan, stage, rep.n_ilp, rep.n_leaves_in, rep.n_children,
                               nRadarMeas, rep.n_leaves_out, rep.n_clusters, rep.n_branched, rep.blp_iters_max, rep.n_limit, used_raw,
                               len(self._tbl_), time.time() - t_init, total))
        if len(self._scanrecs) >= 256:      # (a host that streams for hours without reading toc / runtimeLog: the tuples -- each holds its scan's tic and used-measurement words -- do not pile up)
            self._materialise()
        if total > self.radarPeriod * 0.6 or tic.get('_print'):
            self._materialise()
            if total > 0.1 and os.environ.get("MHT_STALL_DEBUG") == "1":      # (development: which part of a scan was slow)
                self._stall_debug(scanNumber, call, now - t_fold)
            if total > self.radarPeriod:
                log.critical("Did not pass real time demand! Used {0:.0f}ms of {1:.0f}ms".format(total * 1000, self.radarPeriod * 1000))
            elif total > self.radarPeriod * 0.6:      # tracker.py:285-287
                log.warning("Did almost not pass real time demand! Used {0:.0f}ms of {1:.0f}ms".format(total * 1000, self.radarPeriod * 1000))
            # the reference's per-scan console output (tracker.py:222-223, :296-301), when the scan is folded
            kw = tic.get('_print')
            if kw:
                if kw.get("printCluster", False):
                    self.printClusterList(self.__clusterList__)
                if kw.get("printInfo", False):
                    print("Added scan number:", len(self.__scanHistory__), " \tnRadarMeas ", nRadarMeas, sep="")
                if kw.get("printTime", False):
                    self.printTimeLog(**kw)

    @staticmethod
    def _unused_of(used_raw, nRadarMeas):
        """bit j of the report's used-measurement words -> unused[j]"""
        return ~np.unpackbits(np.frombuffer(used_raw, dtype=np.uint8), bitorder="little")[:nRadarMeas].astype(bool)

    def _materialise(self):
        """The per-scan tuples `_finish_scan` left -> the reference's `toc` / `runtimeLog` / `lastScanStats` (and the scan log)."""
        recs, self._scanrecs = self._scanrecs, []
        if len(recs) > 1:
            # all but the newest scan only add a row to `runtimeLog` (and to the scan log when it is kept); `toc`, `tic`, `lastScanStats` are the newest
            # scan's.  One pass per column instead of a dictionary per scan: a streaming host pays 0.5 us per scan for this, not 2.7 (it runs every
            # 256 scans, in the middle of the stream)
            older = recs[:-1]
            rl = self._runtimeLog_
            rl['Total'].extend(r[18] for r in older)
            rl['Init'].extend(r[17] for r in older)
            rl['Process'].extend(r[1] * 1e-8 if r[5] is None else r[5][0] for r in older)
            rl['Cluster'].extend(r[2] * 1e-8 if r[5] is None else r[5][1] for r in older)
            rl['Optim'].extend(r[3] * 1e-8 if r[5] is None else r[5][2] for r in older)
            rl['N-Prune'].extend(0.0 if r[5] is None else r[5][3] for r in older)
            zeros = [0.0] * len(older)
            for k in ('ILP-Prune', 'DynN', 'Terminate'):
                rl[k].extend(zeros)
            if self._scanStatsLog is not None:
                for r in older:
                    self._scanStatsLog.append(dict(L=r[7], G=r[8] - r[7], M=r[9], leaves_out=r[10], clusters=r[11], ilp=r[6], branched=r[12], blp_iters_max=r[13],
                                                   limit=r[14], unused=self._unused_of(r[15], r[9]), nTargets=r[16]))
            recs = recs[-1:]
        for (tic, t_process, t_cluster, t_optim, t_scan, stage, n_ilp, n_leaves_in, n_children, nRadarMeas, n_leaves_out, n_clusters, n_branched,
             blp_iters_max, n_limit, used_raw, n_tbl, t_init, total) in recs:
            self.tic = tic
            # Per-stage times (tracker.py:192-294: the reference's own per-scan metric).  The kernels stamp the GPU's wall clock (10 ns
            # ticks) at the start of every stage and the commit files the differences in the report: no HIP events, no host cost, present
            # on every scan.  Track termination and the N-scan prune decision are part of the ILP launch (toc['Optim']); the target-side
            # commit rides in the next scan's grow launch (toc['N-Prune'] = 0 unless deviceTiming measures it with HIP events).
            toc = {'Process': t_process * 1e-8, 'Cluster': t_cluster * 1e-8, 'Optim': t_optim * 1e-8, 'Terminate': 0.0, 'N-Prune': 0.0,
                   'Device': t_scan * 1e-8, 'ILP-Prune': 0.0, 'DynN': 0.0, 'Init': t_init, 'Total': total}
            if stage is not None:
                toc['Process'], toc['Cluster'], toc['Optim'], toc['N-Prune'], toc['Device'] = stage
            self._toc_ = toc
            self._nOptimSolved_ = n_ilp
            for k, v in self._runtimeLog_.items():
                if k in toc:
                    v.append(toc[k])
            self._stats_ = dict(L=n_leaves_in, G=n_children - n_leaves_in, M=nRadarMeas, leaves_out=n_leaves_out, clusters=n_clusters, ilp=n_ilp,
                                branched=n_branched, blp_iters_max=blp_iters_max, limit=n_limit, unused=self._unused_of(used_raw, nRadarMeas))
            if self._scanStatsLog is not None:
                self._scanStatsLog.append(dict(self._stats_, nTargets=n_tbl))

    def _stall_debug(self, scanNumber, call, fold):
        self._materialise()
        t = self._toc_
        log.critical("scan %d slow: call %.1f ms, device %.1f ms (process %.1f, cluster %.1f, optim %.1f), fold + wait %.1f ms", scanNumber,
                     1e3 * call, 1e3 * t['Device'], 1e3 * t['Process'], 1e3 * t['Cluster'], 1e3 * t['Optim'], 1e3 * fold)
        dbg = np.zeros(8, dtype=np.uint64)
        self._lib.mht_forest_debug_read(self._ctx.handle, b"init_dbg", dbg.ctypes.data_as(C.c_void_p), 64)
        log.critical("init_dbg %s at t = %.1f s (process clock), pid %d", dbg.tolist(), time.process_time(), os.getpid())
        st2 = np.zeros(16, dtype=np.uint64)
        self._lib.mht_forest_debug_read(self._ctx.handle, b"status2", st2.ctypes.data_as(C.c_void_p), 128)
        log.critical("status2 words (overflow | n_children << 32, n_dead | timeout bits << 32): %s %s", [hex(int(x)) for x in st2[:2]], [hex(int(x)) for x in st2[8:10]])

    def _apply_births(self, births, scanTime, scanNumber, z_unused):
        """The device initiator's candidates that Tracker.initiateTarget's device twin admitted: append them to the host mirror."""
        ok = births["id"] >= 0
        if not ok.any():
            return
        b = births[ok]
        n = len(b)
        x0 = b["x0"].astype(np.float32)
        rows = np.zeros(n, dtype=self._REPORT_DTYPE)
        rows["id"], rows["root_scan"], rows["root_node"], rows["root_meas"], rows["root_x"] = b["id"], scanNumber, -1, b["meas"], b["x0"]
        self._tbl_ = np.concatenate([self._tbl_, rows])
        for i in range(n):
            m = int(b["meas"][i])
            self._birth[int(b["id"][i])] = (scanTime, scanNumber, x0[i], b["P0"][i].reshape(self.nx, self.nx).copy(), (m if m > 0 else None),
                                            (z_unused[m - 1] if m > 0 else None), activeTag)
        self.trackIdCounter = int(b["id"].max()) + 1
        self._views.clear()

    def _apply_report(self, recs, scanTime, scanNumber, z, all_alive=None):
        """Fold the scan report into the host tables (no per-target Python objects, no per-field copies: the table of the live
        targets IS the report's rows)."""
        prev = self._tbl_
        if self._views:
            self._views.clear()
        self._labels_src = recs
        alive = None
        if all_alive is None:
            alive = recs["status"] == 0
            all_alive = bool(alive.all())
        if all_alive:
            live = recs
            moved = live["root_scan"] != prev["root_scan"]
        else:
            if alive is None:
                alive = recs["status"] == 0
            # terminated tracks keep their whole history (the reference's _pruneEverythingExceptHistory): the window ancestors of the
            # last selected node are fetched now, while they are still in the device ring
            dead = recs[~alive]
            # (ONE gather launch queued behind the scans in flight, fetched two folds later -- it has long arrived then -- or by whoever
            # looks at the terminated tracks first: a fetch per track stopped the stream for a round trip through the device, 130 us each)
            ticket = C.c_int64(0)
            start = np.ascontiguousarray(dead["sel_node"], dtype=np.int32)
            _lib.check(self._lib.mht_forest_chains_begin(self._ctx.handle, scanNumber, start.ctypes.data_as(C.c_void_p), len(start), self._cfg.n_scan + 2,
                                                         1 if self._ais else 0, C.byref(ticket)))
            entry = [dead, scanTime, scanNumber, z, None, ticket.value, self._fold_no]
            self._dead_chunks.append(entry)
            self._chain_pending.append(entry)
            live = recs[alive]
            moved = live["root_scan"] != prev["root_scan"][alive]
        if moved.any():      # the root of these targets advanced: the new roots join the committed history
            chunk = live if moved.all() else live[moved]
            self._history.append(chunk)
            if self._ais:        # their identities (pyTarget.py:34: Target.mmsi), read while their layers are still in the device ring
                mm = np.zeros(len(chunk), dtype=np.int64)
                # (no message in the last n_scan + 4 scans: no node of the window was updated with one -- nothing to read)
                if scanNumber - self._last_ais_scan <= self._cfg.n_scan + 4:
                    for sc in np.unique(chunk["root_scan"]):
                        if sc >= 1 and scanNumber - int(sc) < self._cfg.n_scan + 3:
                            rows = np.where((chunk["root_scan"] == sc) & (chunk["root_node"] >= 0))[0]
                            if len(rows):      # a gather of these nodes on the device (they sit all over the layer's index space)
                                nodes = np.ascontiguousarray(chunk["root_node"][rows], dtype=np.int32)
                                got = np.zeros(len(rows), dtype=np.int32)
                                _lib.check(self._lib.mht_forest_read_mmsi_nodes(self._ctx.handle, int(sc), len(rows), nodes.ctypes.data_as(C.c_void_p),
                                                                                got.ctypes.data_as(C.c_void_p), None))
                                mm[rows] = got
                self._history_mmsi.append(mm)
        self._tbl_ = live
        self._sel_ = (live, scanTime, scanNumber, z)

    # ---- results: every look at them first folds the report that is still in flight ---------------------------------------
    @property
    def lastScanStats(self):
        self._drain()
        if self._scanrecs:
            self._materialise()
        return self._stats_

    @property
    def scanStatsLog(self):
        self._drain()
        if self._scanrecs:
            self._materialise()
        return self._scanStatsLog

    @property
    def toc(self):
        self._drain()
        if self._scanrecs:
            self._materialise()
        return self._toc_

    @property
    def runtimeLog(self):
        self._drain()
        if self._scanrecs:
            self._materialise()
        return self._runtimeLog_

    @property
    def nOptimSolved(self):
        self._drain()
        if self._scanrecs:
            self._materialise()
        return self._nOptimSolved_

    @property
    def _sel(self):
        self._drain()
        return self._sel_

    @property
    def _tbl(self):
        self._drain()
        return self._tbl_

    # ---- lazily built views (the reference's attributes, tracker.py:74-84) -----------------------------------------
    def _mmsi_layer(self, scanNumber):
        """AIS forest: (mmsi, bound identity) of every node of a layer of the window, read once per scan and cached with the views."""
        key = ("_mmsi", scanNumber)
        v = self._views.get(key)
        if v is None:
            n = int(self._cfg.max_nodes)
            mm, hist = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            _lib.check(self._lib.mht_forest_read_mmsi(self._ctx.handle, int(scanNumber), 0, n, mm.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p)))
            v = self._views[key] = (mm, hist)
        return v

    def _node_view(self, r, scanTime, scanNumber, z):
        m = int(r["sel_meas"])
        mmsi = hist = None
        if self._ais and int(r["sel_node"]) >= 0 and scanNumber == len(self.__scanHistory__):
            layer = self._mmsi_layer(scanNumber)
            mm, hist = int(layer[0][int(r["sel_node"])]), (int(layer[1][int(r["sel_node"])]) or None)
            if mm:
                mmsi, m = mm, (m if m > 0 else None)      # (an AIS-updated node without a radar measurement: measurementNumber None, tracker.py:520)
        node = DeviceTarget(scanTime, scanNumber, np.array(r["sel_x"]), self.P_0, ID=int(r["id"]), P_d=self.default_P_d,
                            measurementNumber=m, measurement=(z[m - 1] if m else None), mmsi=mmsi,
                            cumulativeNLLR=float(r["sel_cnllr"]), status=_STATUS_TAG[int(r["status"])])
        node._tracker, node._node, node._hist_mmsi = self, int(r["sel_node"]), hist
        node._P_lazy = int(r["sel_node"]) >= 0
        node._lazy_parent = self._make_parent_loader(int(r["id"]))
        return node

    @property
    def __trackNodes__(self):
        self._drain()
        v = self._views.get("track")
        if v is None:
            v = np.empty(len(self._tbl_["id"]), dtype=np.dtype(object))
            if self._sel_ is not None and len(self._sel_[0]) == len(v):
                live, scanTime, scanNumber, z = self._sel_
                for i in range(len(live)):
                    v[i] = self._node_view(live[i], scanTime, scanNumber, z)
                n0 = len(live)
            else:
                n0 = 0 if self._sel_ is None else len(self._sel_[0])
                if self._sel_ is not None:
                    live, scanTime, scanNumber, z = self._sel_
                    for i in range(n0):
                        v[i] = self._node_view(live[i], scanTime, scanNumber, z)
            roots = self.__targetList__
            for i in range(n0, len(v)):      # targets born after the last scan: their node is the root itself
                v[i] = roots[i]
            self._views["track"] = v
        return v

    @property
    def __targetList__(self):
        self._drain()
        v = self._views.get("roots")
        if v is None:
            tb = self._tbl_
            v = []
            for i in range(len(tb["id"])):
                tid = int(tb["id"][i])
                b = self._birth.get(tid)
                if b is not None and int(tb["root_scan"][i]) == b[1]:      # still the root it was born with
                    root = DeviceTarget(b[0], b[1], b[2], b[3], ID=tid, P_d=self.default_P_d, measurementNumber=b[4],
                                        measurement=b[5], status=b[6])
                else:
                    rs, rm, r_mmsi, r_hist = int(tb["root_scan"][i]), int(tb["root_meas"][i]), None, None
                    if self._ais and rs >= 1 and int(tb["root_node"][i]) >= 0 and len(self.__scanHistory__) - rs < self._cfg.n_scan + 4:
                        layer = self._mmsi_layer(rs)      # (the root's own identity and the one its track is bound to: per node on the device)
                        mm, r_hist = int(layer[0][int(tb["root_node"][i])]), (int(layer[1][int(tb["root_node"][i])]) or None)
                        if mm:
                            r_mmsi, rm = mm, (rm if rm > 0 else None)
                    root = DeviceTarget(float(self._scan_times[max(rs, 0)]), rs, tb["root_x"][i].copy(), self.P_0,
                                        ID=tid, P_d=self.default_P_d, measurementNumber=rm, mmsi=r_mmsi,
                                        cumulativeNLLR=float(tb["root_cnllr"][i]))
                    root._hist_mmsi = r_hist
                    root._lazy_parent = self._history_parent_loader(tid)
                root.isRoot, root._tracker, root._node = True, self, int(tb["root_node"][i])
                v.append(root)
            self._views["roots"] = v
        return v

    @property
    def __clusterList__(self):
        self._drain()
        labels = self._labels_src["cluster"] if self._labels_src is not None else self._labels
        return [np.where(labels == lab)[0] for lab in np.unique(labels)]

    @property
    def __terminatedTargets__(self):
        self._drain()
        self._resolve_chains()
        out = []
        for recs, scanTime, scanNumber, z, chains, _, _ in self._dead_chunks:
            for r, chain in zip(recs, chains):
                v = self._node_view(r, scanTime, scanNumber, z)
                tid, rs = int(r["id"]), int(r["root_scan"])
                hist = [c for c in self._history_chain(tid) if c.scanNumber <= rs]      # committed roots up to the root it died with
                self._link_chain(v, tid, chain, rs, int(r["root_node"]), hist[-1] if hist else None)
                out.append(v)
        return out

    @property
    def __targetWindowSize__(self):
        self._drain()
        return [self.N] * len(self._tbl_["id"])

    @property
    def __associatedMeasurements__(self):
        self._drain()
        """The association sets live on the device as (target, measurement node) edges; the host view is rebuilt from
        the leaves' ancestor chains on demand (slow path, for inspection only)."""
        return [root.getMeasurementSet() if root.trackHypotheses is not None else set() for root in self.__targetList__]

    # ------------------------------------------------------------------------------------------------
    def _history_chain(self, target_id):
        """Committed roots of one track, oldest first, as Target views linked through `parent`."""
        b = self._birth.get(target_id)
        chain = []
        if b is not None:
            first = DeviceTarget(b[0], b[1], b[2], b[3], ID=target_id, P_d=self.default_P_d, measurementNumber=b[4],
                                 measurement=b[5], status=b[6])
            first._tracker = self
            chain.append(first)
        for ci, ch in enumerate(self._history):
            for k in np.where(ch["id"] == target_id)[0]:
                sc = int(ch["root_scan"][k])
                zz = self.__scanHistory__[sc - 1].measurements if sc >= 1 else None
                m = int(ch["root_meas"][k])
                mmsi = None
                if self._ais and ci < len(self._history_mmsi) and int(self._history_mmsi[ci][k]):
                    mmsi, m = int(self._history_mmsi[ci][k]), (m if m > 0 else None)      # (an AIS-updated node without a radar measurement: measurementNumber None)
                v = DeviceTarget(float(self._scan_times[max(sc, 0)]), sc, ch["root_x"][k].copy(), self.P_0, ID=target_id, P_d=self.default_P_d,
                                 measurementNumber=m, measurement=(np.asarray(zz)[m - 1] if (zz is not None and m) else None), mmsi=mmsi,
                                 cumulativeNLLR=float(ch["root_cnllr"][k]))
                v._tracker, v._node = self, int(ch["root_node"][k])
                v.parent = chain[-1] if chain else None
                chain.append(v)
        return chain

    def _history_parent_loader(self, target_id):
        def load(view):
            chain = self._history_chain(target_id)
            older = [c for c in chain if c.scanNumber < view.scanNumber]
            return older[-1] if older else None
        return load

    def _window_chain(self, scan, node):
        """The ancestors of (scan, node) that are still in the device ring: arrays nodes, meas, x, cnllr, P (index 0 = the node)."""
        n_max = self._cfg.n_scan + 2
        nodes = np.zeros(n_max, dtype=np.int32)
        meas = np.zeros(n_max, dtype=np.int32)
        x = np.zeros((n_max, self.nx))
        cn = np.zeros(n_max)
        n = C.c_int32(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        if self._ais:      # covariances in the dtype the reference gives every node: float64 behind an AIS update (MHT_F_COV_F64), float32 otherwise
            P64 = np.zeros((n_max, self.nx * self.nx))
            fl = np.zeros(n_max, dtype=np.uint8)
            _lib.check(self._lib.mht_forest_chain_f64(self._ctx.handle, scan, node, n_max, p(nodes), p(meas), p(x), p(cn), p(P64), p(fl), C.byref(n)))
            k = n.value
            return nodes[:k], meas[:k], x[:k], cn[:k], [P64[i] if (fl[i] & _F_COV_F64) else P64[i].astype(np.float32) for i in range(k)]
        P = np.zeros((n_max, self.nx * self.nx), dtype=np.float32)
        _lib.check(self._lib.mht_forest_chain(self._ctx.handle, scan, node, n_max, p(nodes), p(meas), p(x), p(cn), p(P), C.byref(n)))
        k = n.value
        return nodes[:k], meas[:k], x[:k], cn[:k], P[:k]

    def _resolve_chains(self, older_than=None):
        """Take the window chains of terminated tracks out of the library's pinned blocks (mht_forest_chains_fetch): all that are pending,
        or those begun before fold `older_than` (their gather launch ran long ago: no wait)."""
        while self._chain_pending and (older_than is None or self._chain_pending[0][6] < older_than):
            entry = self._chain_pending.pop(0)
            n_max = self._cfg.n_scan + 2
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            chains = []
            for i in range(len(entry[0])):
                nodes = np.zeros(n_max, dtype=np.int32)
                meas = np.zeros(n_max, dtype=np.int32)
                x = np.zeros((n_max, self.nx))
                cn = np.zeros(n_max)
                n = C.c_int32(0)
                if self._ais:      # (dtypes per node as _window_chain)
                    P64 = np.zeros((n_max, self.nx * self.nx))
                    fl = np.zeros(n_max, dtype=np.uint8)
                    _lib.check(self._lib.mht_forest_chains_fetch(self._ctx.handle, entry[5], i, p(nodes), p(meas), p(x), p(cn), p(P64), p(fl), C.byref(n)))
                    k = n.value
                    chains.append((nodes[:k], meas[:k], x[:k], cn[:k], [P64[j] if (fl[j] & _F_COV_F64) else P64[j].astype(np.float32) for j in range(k)]))
                else:
                    P = np.zeros((n_max, self.nx * self.nx), dtype=np.float32)
                    _lib.check(self._lib.mht_forest_chains_fetch(self._ctx.handle, entry[5], i, p(nodes), p(meas), p(x), p(cn), p(P), None, C.byref(n)))
                    k = n.value
                    chains.append((nodes[:k], meas[:k], x[:k], cn[:k], P[:k]))
            entry[4] = chains

    def _link_chain(self, view, target_id, chain, root_scan, root_node, root_view):
        """Hang the window ancestors `chain` under `view`; where the chain reaches (root_scan, root_node) it continues with
        `root_view` (the committed history).  An ancestor at the root's scan that is NOT the root means the view was taken
        before a prune that cut its branch off: the chain ends there (parent None) instead of being joined to a foreign root."""
        nodes, meas, x, cn, P = chain
        if len(P):
            view.P_0 = P[0].reshape(self.nx, self.nx).copy()
        prev = view
        for k in range(1, len(nodes)):
            sc = view.scanNumber - k
            if sc == root_scan:
                prev._parent, prev._lazy_parent = (root_view if int(nodes[k]) == root_node or root_node < 0 else None), None
                return view._parent
            if sc < root_scan:
                break
            zz = self.__scanHistory__[sc - 1].measurements if sc >= 1 else None
            m = int(meas[k])
            mmsi = hist = None
            if self._ais and sc >= 1:      # the ancestor's own identity and the one its track is bound to (pyTarget.py:34, :297-302), per node on the device
                layer = self._mmsi_layer(sc)
                mm, hist = int(layer[0][int(nodes[k])]), (int(layer[1][int(nodes[k])]) or None)
                if mm:
                    mmsi, m = mm, (m if m > 0 else None)
            a = DeviceTarget(self.__scanHistory__[sc - 1].time if sc >= 1 else view.time, sc, x[k].copy(),
                             P[k].reshape(self.nx, self.nx).copy(), ID=target_id, P_d=self.default_P_d, measurementNumber=m,
                             measurement=(np.asarray(zz)[m - 1] if (zz is not None and m) else None), mmsi=mmsi,
                             cumulativeNLLR=float(cn[k]))
            a._tracker, a._node, a._hist_mmsi = self, int(nodes[k]), hist
            prev._parent, prev._lazy_parent = a, None
            prev = a
        prev._lazy_parent = None
        return view._parent

    def _make_parent_loader(self, target_id):
        def load(view):
            # ancestors inside the device window, then the committed root history kept on the host
            if len(self.__scanHistory__) - view.scanNumber >= self._cfg.n_scan + 4:      # (the device ring holds N+4 scans: mht_forest.hip RING_EXTRA)
                return None
            chain = self._window_chain(view.scanNumber, view._node)
            hit = np.where(self._tbl_["id"] == target_id)[0]
            if len(hit) == 0:
                return self._link_chain(view, target_id, chain, -1, -1, None)
            i = int(hit[0])
            return self._link_chain(view, target_id, chain, int(self._tbl_["root_scan"][i]), int(self._tbl_["root_node"][i]),
                                    self.__targetList__[i])
        return load

    def _leaf_snapshot(self):
        """All leaves of the forest, exported once per scan: cached with the other lazily built views (dropped by the next scan or
        birth), sized by the report's leaf count rather than by max_nodes (`Target.getLeafNodes` of every root goes through here)."""
        self._drain()
        snap = self._views.get("_leaves")
        if snap is not None:
            return snap
        leaves_out = self._scanrecs[-1][10] if self._scanrecs else self._stats_.get("leaves_out", 0)
        cap = int(min(self._cfg.max_nodes, max(4096, 2 * int(leaves_out) + 4 * len(self._tbl_) + 1024)))
        while True:
            snap = self._leaf_export(cap)
            if snap is not None:
                break
            cap = self._cfg.max_nodes
        self._views["_leaves"] = snap
        return snap

    def _leaf_export(self, cap):
        n = C.c_int32(0)
        x = np.zeros((cap, self.nx)); cn = np.zeros(cap)
        P = np.zeros((cap, self.nx * self.nx), dtype=np.float64 if self._ais else np.float32)
        meas = np.zeros(cap, dtype=np.int32); tgt = np.zeros(cap, dtype=np.int32); ids = np.zeros(cap, dtype=np.int32)
        node = np.zeros(cap, dtype=np.int32); fl = np.zeros(cap, dtype=np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        # (AIS forest: every covariance as float64 -- exact for the float32 ones; "Pf64" tells which leaves the reference carries in float64)
        export = self._lib.mht_forest_leaves_f64 if self._ais else self._lib.mht_forest_leaves
        _lib.check(export(self._ctx.handle, cap, p(x), p(P), p(cn), p(meas), p(tgt), p(ids), p(node), p(fl), C.byref(n)))
        if n.value > cap and cap < self._cfg.max_nodes:
            return None      # (more leaves than the estimate -- the export is truncated to the capacity: the caller retries with the full one)
        k = min(n.value, cap)
        out = dict(x=x[:k], P=P[:k].reshape(k, self.nx, self.nx), cnllr=cn[:k], meas=meas[:k], target=tgt[:k], ID=ids[:k],
                   node=node[:k], flags=fl[:k])
        if self._ais:      # identities; a node with one and no radar measurement gets meas = -1 (measurementNumber None)
            out["Pf64"] = (out["flags"] & _F_COV_F64) != 0
            scan = len(self.__scanHistory__)
            out["mmsi"] = self._mmsi_layer(scan)[0][out["node"]].astype(np.int64) if scan > 0 else np.zeros(k, dtype=np.int64)
            out["meas"] = np.where((out["meas"] == 0) & (out["mmsi"] != 0), -1, out["meas"]).astype(np.int32)
        return out

    def leafBatch(self):
        """All current leaves in target-list / DFS order (what the next scan will gate): dict of arrays."""
        return dict(self._leaf_snapshot())

    def _leaf_views(self, root):
        snap = self._leaf_snapshot()
        scan = len(self.__scanHistory__)
        t = self.__scanHistory__[-1].time if scan else root.time
        out = []
        for i in np.where(snap["ID"] == root.ID)[0]:
            if int(snap["node"][i]) == root._node and root.scanNumber == scan:
                out.append(root)
                continue
            m, mmsi = int(snap["meas"][i]), None
            if self._ais and int(snap["mmsi"][i]):
                mmsi, m = int(snap["mmsi"][i]), (m if m > 0 else None)
            Pi = snap["P"][i].copy() if (not self._ais or snap["Pf64"][i]) else snap["P"][i].astype(np.float32)
            v = DeviceTarget(t, scan, snap["x"][i].copy(), Pi, ID=root.ID, P_d=self.default_P_d,
                             measurementNumber=m, mmsi=mmsi, cumulativeNLLR=float(snap["cnllr"][i]))
            v._tracker, v._node = self, int(snap["node"][i])
            v._lazy_parent = self._make_parent_loader(root.ID)
            out.append(v)
        return out

    # ------------------------------------------------------------------------------------------------
    @property
    def nTargets(self):
        """len(__targetList__) without building the views."""
        self._drain()
        return len(self._tbl_["id"])

    def getTrackNodes(self):
        return self.__trackNodes__

    def _ais_message(self, scanNumber, mmsi):
        """The message of ship `mmsi` among those handed in with scan `scanNumber` (1-based: _finish_scan appends a scan's list to
        __aisHistory__ as it appends the scan to __scanHistory__, so scan n is entry n - 1 of both), or None."""
        hist = self.__aisHistory__
        if scanNumber is None or not 1 <= scanNumber <= len(hist):
            return None
        for m in (hist[scanNumber - 1] or ()):
            if m.mmsi == mmsi:
                return m
        return None

    def _ais_lookup(self, constantTurn=False):
        """What ais=True hands to smoothing.smooth_nodes; ValueError where the switch does not apply."""
        if constantTurn:
            raise ValueError("ais=True and constantTurn=True exclude each other: AIS messages report four states of a linear model")
        if not self._ais:
            raise ValueError("ais=True needs a Tracker made with aisAided=True: this one has fused no AIS message")
        self._drain()
        return self._ais_message

    def _smooth_nodes(self, nodes, constantTurn=False, ais=False, em=0, emStart="model"):
        from . import smoothing
        if em and (ais or constantTurn):
            raise ValueError("em learns the noise of the plain linear model: not together with ais=True or constantTurn=True")
        return smoothing.smooth_nodes(self._model_mod, self.radarPeriod, nodes, ctx=self._ctx, constantTurn=constantTurn,
                                      ais=self._ais_lookup(constantTurn) if ais else None, em=em, emStart=emStart)

    def getSmoothTracks(self, terminated=False, constantTurn=False, ais=False, em=0, emStart="model", imm=None):
        """tracker.py: [track.getSmoothTrack(radarPeriod) for track in __trackNodes__] -- (positions, velocities, ok) per live track, with
        terminated=True followed by the terminated ones (__terminatedTargets__) -- smoothed in ONE batched device call
        (pymht_amd/smoothing.py: a Rauch-Tung-Striebel smoother with the tracker's own model, not pykalman).  A constant-turn tracker
        raises NotImplementedError: its transition depends on the state -- unless constantTurn=True asks for the smoother of that model
        (Phi(T, w) at each node's filtered turn rate, no Jacobian: smoothing.smooth_tracks_ct), which in turn raises ValueError for a
        tracker on a linear model.  ais=True (a tracker made with aisAided=True, else ValueError; not with constantTurn): the smoother
        of the model the forest filtered with -- a node that took an AIS message is predicted to the message's time, updated with it
        and predicted on to the scan (smoothing.smooth_tracks_ais), the messages looked up in __aisHistory__; a node whose message is
        not there raises RuntimeError.  By default an AIS-aided tracker's histories are smoothed from their radar plots alone.
        em > 0 (linear models; not with constantTurn or ais: ValueError): Q, R and the initial state are learned per track by `em`
        EM iterations before the smoothing walk (smoothing.smooth_tracks_em); emStart="reference" starts them at the identity as the
        reference's pykalman call does, so that em=5, emStart="reference" is the reference's procedure, restated.  ok is False for a
        track whose learned covariances stopped being positive definite (its output is NaN).
        imm: None, or a tuple of scales of Q (getSmoothModeProbabilities' qScales, with its default `stay`): positions and velocities
        are then the IMM smoother's combined state (smoothing.imm_smooth_nodes), which needs no choice of a single noise level; not
        together with ais=True or em > 0 (ValueError).  A chain of fewer than two nodes is answered as without imm."""
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        if imm is not None:
            if ais or em:
                raise ValueError("imm smooths under several noise levels of the tracker's model: not together with ais=True or em > 0")
            out = []
            for node, d in zip(nodes, self._imm_smooth_nodes(nodes, imm, 0.95, constantTurn)):
                if len(d["x"]) < 2:      # (nothing to smooth: its measurements, NaN velocities, False -- no device call)
                    out.append(self._smooth_nodes([node], constantTurn=constantTurn)[0])
                else:
                    out.append((d["x"][:, 0:2], d["x"][:, 2:4], True))
            return out
        return self._smooth_nodes(nodes, constantTurn=constantTurn, ais=ais, em=em, emStart=emStart)

    def getFilteredTracks(self, terminated=False, constantTurn=False, ais=False):
        """The filtered state and covariance along every track history: (xf [L, nx], Pf [L, nx, nx]) per live track, in the order of
        getSmoothTracks, with terminated=True followed by the terminated ones -- ONE forward-only device call
        (smoothing.filter_nodes / filter_tracks).  These are the states of the float64 filter the smoothers and the scores run: the
        tracker's model over the history from the chain's initial state -- the forward half of getSmoothTracks bit for bit, and NOT
        the forest's own float32 / float64 chains bit for bit (a node's P_0 keeps returning the forest's covariance while the node
        is in the ring, and None afterwards).  constantTurn and ais as for getSmoothTracks, with the same refusals."""
        from . import smoothing
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        return smoothing.filter_nodes(self._model_mod, self.radarPeriod, nodes, ctx=self._ctx, constantTurn=constantTurn,
                                      ais=self._ais_lookup(constantTurn) if ais else None)

    def getModeProbabilities(self, qScales=(1.0, 16.0), stay=0.95, terminated=False, constantTurn=False):
        """WHERE along each track a louder model takes over: an interacting-multiple-model filter over every track history, one mode per
        entry of qScales (up to four; mode j runs the tracker's model with qScales[j] times its Q, the chain between the modes keeps
        a mode with probability `stay`: smoothing.imm_modes), in ONE device call (smoothing.imm_nodes / imm_tracks, which define the
        figures).  One dict per live track, in the order of getSmoothTracks, with terminated=True followed by the terminated ones:
        mu [L, r] the probability of every mode at every node -- a manoeuvre detector per track and scan --, x [L, nx] and P [L, nx, nx]
        the combined state and covariance in getFilteredTracks' layout, logLikelihood and nObs as getTrackLikelihoods defines them,
        under the mixture.  With qScales=(1.0,) they are getFilteredTracks' and getTrackLikelihoods' figures bit for bit.  The default
        scales are a starting point, NOT tuned: getLikelihoodSurface says which single level fits, and a second level several times
        louder is what a turn needs.  The refusals are getFilteredTracks': a constant-turn tracker raises NotImplementedError without
        constantTurn=True, which raises ValueError for a tracker on a linear model; AIS messages are not taken."""
        from . import smoothing
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        (smoothing._check_ct_model if constantTurn else smoothing._check_model)(self._model_mod)
        Q, R, Pi, mu0 = smoothing.imm_modes(self._model_mod, self.radarPeriod, qScales, stay=stay)
        per, ll, nobs = smoothing.imm_nodes(self._model_mod, self.radarPeriod, nodes, Q, R, Pi, mu0, ctx=self._ctx, constantTurn=constantTurn)
        return [dict(mu=mu, x=x, P=P, logLikelihood=float(a), nObs=int(b)) for (mu, x, P), a, b in zip(per, ll, nobs)]

    def _imm_smooth_nodes(self, nodes, qScales, stay, constantTurn):
        from . import smoothing
        (smoothing._check_ct_model if constantTurn else smoothing._check_model)(self._model_mod)
        Q, R, Pi, mu0 = smoothing.imm_modes(self._model_mod, self.radarPeriod, qScales, stay=stay)
        return smoothing.imm_smooth_nodes(self._model_mod, self.radarPeriod, nodes, Q, R, Pi, mu0, ctx=self._ctx, constantTurn=constantTurn)

    def getSmoothModeProbabilities(self, qScales=(1.0, 16.0), stay=0.95, terminated=False, constantTurn=False):
        """getModeProbabilities IN HINDSIGHT: the fixed-interval IMM smoother over every track history (smoothing.imm_smooth_nodes /
        imm_smooth_tracks, which define the figures), in ONE device call.  The filter says where a louder model takes over several
        scans late, at the start of a turn and again at its end; the smoother has seen the scans behind.  One dict per track, in
        getModeProbabilities' order and with its arguments and refusals: mu [L, r] the smoothed probability of every mode, muFiltered
        [L, r] getModeProbabilities' own, x [L, nx] and P [L, nx, nx] the smoothed combined state and covariance in getFilteredTracks'
        layout (what evaluation.nees_nodes takes as they are), logLikelihood and nObs as getModeProbabilities gives them.  With
        qScales=(1.0,) x and P are the smoother's own (smoothing.smooth_tracks).  The default scales are a starting point, NOT tuned."""
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        return self._imm_smooth_nodes(nodes, qScales, stay, constantTurn)

    def getTrackLikelihoods(self, terminated=False, constantTurn=False, ais=False):
        """How well the tracker's model explains each track's plots: (logLikelihood, nis, nObs) per live track, in the order of
        getSmoothTracks, with terminated=True followed by the terminated ones -- scored in ONE forward-only device call
        (smoothing.score_nodes / score_tracks, which define the figures: node 0 is the initial state and no observation; nis, the
        normalised innovation squared summed over the track's nObs plots, is chi-square with 2 nObs degrees of freedom when the filter
        is consistent -- the figure to tune sigmaQ and R by).  constantTurn and ais as for getSmoothTracks, with the same refusals: a
        constant-turn tracker raises NotImplementedError without constantTurn=True, ais=True needs an AIS-aided tracker and excludes
        constantTurn (ValueError); with ais=True each tuple is (logLikelihood, nis, nObs, nisAis, nAis), the messages scored too."""
        from . import smoothing
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        return smoothing.score_nodes(self._model_mod, self.radarPeriod, nodes, ctx=self._ctx, constantTurn=constantTurn,
                                     ais=self._ais_lookup(constantTurn) if ais else None)

    def getTrackInnovations(self, terminated=False, constantTurn=False, ais=False):
        """getTrackLikelihoods with its terms handed out per node: one dict of NumPy arrays per track, in getTrackLikelihoods' order --
        v [L, 2], S [L, 2, 2], nis [L], ll [L], observed [L] (and with ais=True vAis [L, 4], SAis [L, 4, 4], nisAis [L], llAis [L],
        message [L]), NaN rows where a node has no plot (no message): the innovation sequence of the tracker's filter, which says WHERE
        on a track the model stops fitting (smoothing.trace_nodes / trace_tracks define the figures; one device call).  Added up in
        node order they are getTrackLikelihoods' sums bit for bit.  terminated, constantTurn and ais as there, with the same refusals."""
        from . import smoothing
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        return smoothing.trace_nodes(self._model_mod, self.radarPeriod, nodes, ctx=self._ctx, constantTurn=constantTurn,
                                     ais=self._ais_lookup(constantTurn) if ais else None)

    def getConsistency(self, alpha=0.05, terminated=False, constantTurn=False, ais=False):
        """The filter-consistency statistics of the tracks' radar innovations, pooled over getTrackInnovations' traces
        (smoothing.consistency: the time-average NIS against its chi-square interval, the share of outliers, the lag-one
        autocorrelation of the whitened innovations against its bound); alpha is the tests' size."""
        from . import smoothing
        return smoothing.consistency(self.getTrackInnovations(terminated=terminated, constantTurn=constantTurn, ais=ais), alpha=alpha)

    def _step_estimates(self, nodes, times, smooth, constantTurn, ais):
        """The estimates getGospa and getNees hold against the truth of each step: (X, ids, nIgnored, where) -- per step the positions
        [k, 2] of the nodes with that time stamp on the histories of `nodes` (the forest's filtered positions, or getSmoothTracks'
        with smooth), their track IDs, the nodes at no step's time, and per step the (history, node) indices of the estimates."""
        smoothed = self._smooth_nodes(nodes, constantTurn=constantTurn, ais=ais) if smooth else None
        step_of = {}
        for s, t in enumerate(times):
            step_of.setdefault(float(t), s)
        X, ids, where, nIgnored = [[] for _ in times], [[] for _ in times], [[] for _ in times], 0
        for i, leaf in enumerate(nodes):
            chain = leaf.backtrackNodes()
            tid = leaf.ID if leaf.ID is not None else chain[0].ID if chain[0].ID is not None else -(i + 1)
            for k, node in enumerate(chain):
                s = step_of.get(float(node.time))
                if s is None:
                    nIgnored += 1
                    continue
                pos = smoothed[i][0][k] if smooth and len(chain) >= 2 else node.x_0[0:2]      # (a chain of one node has nothing to smooth)
                X[s].append(np.asarray(pos, dtype=np.float64).reshape(2))
                ids[s].append(tid)
                where[s].append((i, k))
        return [np.array(x, dtype=np.float64).reshape(-1, 2) for x in X], ids, nIgnored, where

    def getGospa(self, truth, c, p=2, terminated=True, smooth=False, constantTurn=False, ais=False):
        """The track histories scored against ground truth: GOSPA per step (evaluation.gospa_steps, which defines the figures; one
        device launch for all steps), the one figure here that says whether the tracker FOUND the targets -- missed targets, false
        tracks and track switches, which no likelihood sees.

        truth   a sequence of (time, positions [m, >= 2]), or a pair (times, positions per time) such as
                (sc["times"], sc["truth"]) of a scenario; only the first two columns of the positions are read
        c, p    GOSPA's cut-off and exponent (1 or 2)
        The steps are the truth's times.  The estimates of a step are the positions of the nodes with that time stamp (compared with
        == on the float the MeasurementList carried) on the track histories of __trackNodes__, with terminated=True (the default)
        also of __terminatedTargets__; nodes at other times -- the initial state of a track is one -- are left out and counted in
        nIgnored.  smooth=True: the positions are getSmoothTracks' instead of the filtered ones, constantTurn and ais select that
        call's smoother and carry its refusals (without smooth=True they are refused: ValueError).

        THESE ARE THE HISTORIES AS THEY STAND AT THE CALL: resolved by the N-scan window, every track one chain.  They are not the
        estimates the tracker reported online at each scan, which a hypothesis pruned since may have produced.

        Returns gospa_steps' dict (gospa, total, localisation, missed, false, nAssigned, nMissed, nFalse over the steps, match per
        step) plus times, trackIds (per step the track ID of every estimate, in the order of match), idSwitches (evaluation.id_switches
        over the truths' rows: (total, perTruth)), nIgnored, and the means over the steps meanGospa, meanLocalisation, meanMissed,
        meanFalse (NaN without steps)."""
        from . import evaluation
        if (constantTurn or ais) and not smooth:
            raise ValueError("getGospa: constantTurn and ais select the smoother of smooth=True; the filtered positions need neither")
        c, p = evaluation._check_cutoff(c, p)
        times, Y = evaluation.truth_steps(truth)
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        X, ids, nIgnored, _ = self._step_estimates(nodes, times, smooth, constantTurn, ais)
        out = evaluation.gospa_steps(X, Y, c, p, ctx=self._ctx)
        out["times"], out["trackIds"], out["nIgnored"] = times, ids, nIgnored
        out["idSwitches"] = evaluation.id_switches(out["match"], ids)
        for key, name in (("gospa", "meanGospa"), ("localisation", "meanLocalisation"), ("missed", "meanMissed"), ("false", "meanFalse")):
            out[name] = float(np.mean(out[key])) if len(times) else float("nan")
        return out

    def getNees(self, truth, c, dims=None, smooth=False, constantTurn=False, ais=False, terminated=True, alpha=0.05):
        """Is the covariance the tracker reports honest?  The estimation error of the track histories against the true STATES and its
        normalised square (NEES) per node, and the chi-square tests on it (evaluation.nees_nodes and nees_consistency define the
        figures) -- the test that sees a velocity bias or a P too small in the unmeasured states, which getConsistency's innovation
        tests, on the two measured coordinates, pass.

        truth   getGospa's two forms; here the columns beyond the first two are read as well: a truth row is the leading components
                [x, y, vx, vy, ...] of the true state, e.g. (sc["times"], sc["truth"]) of utils/scenario.make_scenario ([T, 4] per step)
        c       the cut-off of the pairing: a node is scored against the truth GOSPA (p = 2) assigns it at its step, evaluation.gospa_steps
                on getGospa's own estimates -- the forest's filtered positions, or getSmoothTracks' with smooth=True.  Every other
                node has no truth and is not scored
        dims    2, 4 or the model's state dimension: the components scored.  None: the largest of them every step's truth carries.
                ValueError if a step's truth has fewer columns
        smooth  False: the states scored are getFilteredTracks' (xf, Pf) -- the float64 filter of the smoothers and scores run over
                the history, not the forest's own chains bit for bit.  True: the smoothed (xs, Ps) of smoothing.smooth_tracks*, whose
                covariances nothing else checks; constantTurn and ais select the smoother and carry getSmoothTracks' refusals
                (without smooth=True they are refused: ValueError)
        alpha   the size of nees_consistency's tests

        SELECTION: only pairs closer than c are scored, so a small c cuts the tail off the errors and biases the NEES LOW -- a filter
        looks more honest, or more pessimistic, than it is.  Choose c several standard deviations of the position error wide; then
        the pairs lost are the tracker's misses (getGospa counts them), not the error's tail.

        THESE ARE THE HISTORIES AS THEY STAND AT THE CALL: resolved by the N-scan window, every track one chain.  They are not the
        estimates the tracker reported online at each scan, which a hypothesis pruned since may have produced.

        The filter's (smoother's) outputs stay on the device: only the truth goes up and the figures come down (one mht_nees_nodes
        launch behind the filter's or smoother's one; with smooth=True the pairing runs getSmoothTracks' means-only smoother first).
        Returns a dict: tracks (per history, in getGospa's order, nees_nodes' dict plus step [L], the step of each node or -1),
        trackIds, consistency (nees_consistency's dict), dims, times, nAssigned (the nodes scored), nUnassigned (nodes at a step's
        time that GOSPA left unassigned) and nIgnored (nodes at no step's time)."""
        from . import evaluation, smoothing
        if (constantTurn or ais) and not smooth:
            raise ValueError("getNees: constantTurn and ais select the smoother of smooth=True; the filtered states need neither")
        c, _ = evaluation._check_cutoff(c, 2)
        times, Y = evaluation.truth_steps(truth)
        model = self._model_mod
        nx = int(np.asarray(model.C_RADAR).shape[1])
        Y = [np.asarray(y, dtype=np.float64).reshape(-1, np.shape(y)[1] if np.ndim(y) == 2 else 2) for y in Y]
        cols = min([y.shape[1] for y in Y if len(y)], default=nx)
        allowed = sorted({2, 4, nx})
        if dims is None:
            dims = max([d for d in allowed if d <= cols], default=None)
        if isinstance(dims, bool) or dims not in allowed:
            raise ValueError("getNees: dims is one of %r, the components of the state the truth is held against (got %r)" % (allowed, dims))
        if cols < dims:
            raise ValueError("getNees: dims = %d, and the truth of some step has only %d columns" % (dims, cols))
        dims = int(dims)
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        lookup = self._ais_lookup(constantTurn) if ais else None
        X, ids, nIgnored, where = self._step_estimates(nodes, times, smooth, constantTurn, ais)
        match = evaluation.gospa_steps(X, Y, c, 2, ctx=self._ctx)["match"]
        chains = [smoothing.chain_inputs(node, model.P0) for node in nodes]
        trackIds = [leaf.ID if leaf.ID is not None else ch[0].ID if ch[0].ID is not None else -(i + 1) for i, (leaf, (ch, _)) in enumerate(zip(nodes, chains))]
        out = {"tracks": [], "trackIds": trackIds, "dims": dims, "times": times, "nAssigned": 0, "nUnassigned": 0, "nIgnored": nIgnored}
        if nodes:
            batch = [inp if lookup is None else inp + (smoothing.chain_ais(ch, lookup),) for ch, inp in chains]
            if lookup is not None:
                nx = smoothing._check_ais_model(model)
                extra = dict(ais=smoothing._ais_inputs(model, batch))
                batch = [t[:3] for t in batch]
            else:
                nx = (smoothing._check_ct_model if constantTurn else smoothing._check_model)(model)
                extra = {}
            period = float(self.radarPeriod)
            if smooth:
                x_d, P_d, lens, order, L_max = smoothing._smooth(self._ctx, model, period, batch, nx, True, constantTurn, on_device=True, **extra)
            else:
                x_d, P_d, lens, order, L_max = smoothing._filter(self._ctx, model, period, batch, nx, False, on_device=True)
            n = len(nodes)
            back = np.empty(n, dtype=np.int64)      # history i sits in packed column back[i]
            back[order] = np.arange(n)
            tp, pp = np.zeros((L_max, nx, n)), np.zeros((L_max, n), dtype=np.uint8)
            steps = [np.full(int(L), -1, dtype=np.int64) for L in lens]
            for s, (mt, wh) in enumerate(zip(match, where)):
                for e, (i, k) in enumerate(wh):
                    steps[i][k] = s
                    if mt[e] >= 0:
                        tp[k, :dims, back[i]], pp[k, back[i]] = Y[s][int(mt[e]), :dims], 1
                        out["nAssigned"] += 1
                    else:
                        out["nUnassigned"] += 1
            rows = evaluation._nees_launch(self._ctx, nx, n, L_max, dims, x_d, P_d, tp, pp)
            for i in range(n):
                d = evaluation._nees_dict(np.ascontiguousarray(rows[:lens[i], :, back[i]]), nx)
                d["step"] = steps[i]
                out["tracks"].append(d)
        out["consistency"] = evaluation.nees_consistency(out["tracks"], alpha=alpha)
        return out

    def getEncounters(self, horizon, radius, ownShip=None, ownCovariance=None, steps=None):
        """Which of the live tracks come close to each other -- or to the own ship -- within the next `horizon` seconds, and how sure
        is that?  What a collision-avoidance system asks of a tracker (evaluation.encounters defines the figures): per pair the closest
        point of approach (tcpa, dcpa), the smallest Mahalanobis distance (md2) and the largest probability over the horizon of being
        within `radius` of each other (pc, at time tpc, by the stated rule: good to about 1e-6, not exact).  Times count from the
        current scan.

        horizon, radius   seconds ahead (> 0) and the safety radius (> 0, metres)
        steps       None: ceil(horizon / radarPeriod), at most 64; dt = horizon / steps.  Phi(dt) and Q(dt) are the model module's, in
                    float64
        ownShip     None: all pairs of live tracks.  Else the own ship's state of the model's length, or a position with velocity
                    ([x, y] or [x, y, vx, vy]), padded with zeros: it becomes entry 0, with ownCovariance ([nx, nx], or smaller and
                    padded with zeros; default: zeros, a known own state), and only the own ship against every track is computed
        The entries are the last rows of getFilteredTracks() of every live track, all at the current scan: the states of the float64
        filter over each history.  The AIS-aided filter's state is NOT used, as with getFilteredTracks() by default: an AIS-aided
        tracker's entries are filtered from the radar plots alone.  The tracks are taken as independent (cross-correlation between
        them is not modelled).  A constant-turn tracker raises NotImplementedError (model "ct": its transition depends on the state).
        Returns evaluation.encounters' dict of [first, n] arrays (first = 1 with ownShip, else n) plus `ids`, the targets' ids in entry
        order (None for the own ship).  Fewer than two entries: empty arrays (all NaN) and no device call."""
        from . import evaluation
        for name, v in (("horizon", horizon), ("radius", radius)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
                raise ValueError("getEncounters: %s must be a finite positive number (got %r)" % (name, v))
        if steps is None:
            steps = min(int(np.ceil(float(horizon) / float(self.radarPeriod))), evaluation.ENCOUNTER_MAX_STEPS)
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= evaluation.ENCOUNTER_MAX_STEPS:
            raise ValueError("getEncounters: steps is an integer in 1 .. %d (got %r)" % (evaluation.ENCOUNTER_MAX_STEPS, steps))
        steps = int(steps)
        dt = float(horizon) / steps
        nx, Phi, Q = evaluation.encounter_model(self._model_mod, dt)
        x, P, ids = [], [], []
        if ownShip is not None:
            own = np.asarray(ownShip, dtype=np.float64).reshape(-1)
            if len(own) not in (2, 4, nx):
                raise ValueError("getEncounters: ownShip is [x, y], [x, y, vx, vy] or a state of %d components (got %d)" % (nx, len(own)))
            cov = np.zeros((nx, nx)) if ownCovariance is None else np.asarray(ownCovariance, dtype=np.float64)
            if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] not in (2, 4, nx):
                raise ValueError("getEncounters: ownCovariance is a square matrix of 2, 4 or %d rows (got shape %r)" % (nx, cov.shape))
            xo, Po = np.zeros(nx), np.zeros((nx, nx))
            xo[:len(own)] = own
            Po[:cov.shape[0], :cov.shape[0]] = cov
            x.append(xo)
            P.append(Po)
            ids.append(None)
        elif ownCovariance is not None:
            raise ValueError("getEncounters: ownCovariance without ownShip")
        nodes = list(self.__trackNodes__)
        if nodes:
            from . import smoothing
            chains = [smoothing.chain_inputs(node, self._model_mod.P0)[0] for node in nodes]
            ids += [leaf.ID if leaf.ID is not None else ch[0].ID if ch[0].ID is not None else -(i + 1) for i, (leaf, ch) in enumerate(zip(nodes, chains))]
            for xf, Pf in self.getFilteredTracks():
                x.append(np.asarray(xf, dtype=np.float64)[-1])
                P.append(np.asarray(Pf, dtype=np.float64)[-1])
        n = len(x)
        first = 1 if ownShip is not None else n
        if n < 2:
            out = evaluation._encounter_empty(min(first, n), n)
        else:
            out = evaluation.encounters(np.array(x), np.array(P), Phi, Q, steps, dt, float(radius), first=first, ctx=self._ctx)
        out["ids"] = ids
        return out

    def getTrialManoeuvres(self, horizon, radius, ownShip, courseChanges, turnRate, speedFactors=(1.0,), delay=0.0, ownCovariance=None, steps=None):
        """And if the own ship alters course or speed?  The trial-manoeuvre question of a collision-avoidance system: a grid of candidate
        manoeuvres of the own ship, each held against every live track over the next `horizon` seconds, in one device call
        (evaluation.trial_manoeuvres defines the manoeuvre and the figures).  Times count from the current scan.

        horizon, radius, steps   as for getEncounters: steps None is ceil(horizon / radarPeriod), at most 64; dt = horizon / steps
        ownShip        [x, y, vx, vy]: the own ship's position and velocity at the current scan
        courseChanges  the course changes in radians, positive counter-clockwise in the tracker's axes, |dpsi| <= pi; 0 is "keep the
                       course"
        speedFactors   the speed factors f >= 0 (0.5: half speed); the speed changes at `delay` at once
        delay          seconds >= 0 until the manoeuvre begins, the same for all candidates
        turnRate       the own ship's turn rate in rad/s, > 0.  There is no default: it is the ship's, not the tracker's
        ownCovariance  None (a known own position) or the own ship's 2 x 2 position covariance, constant over the horizon
        The candidates are the product courseChanges x speedFactors, the speed factor fastest: candidate c * len(speedFactors) + s.
        The entries are getEncounters': the last rows of getFilteredTracks() of every live track, all at the current scan.  The
        AIS-aided filter's state is NOT used: an AIS-aided tracker's entries are filtered from the radar plots alone.  The own ship and
        the tracks are taken as independent.  A constant-turn tracker raises NotImplementedError (model "ct": its transition depends on
        the state).
        Returns evaluation.trial_manoeuvres' dict -- the five figures as [G, n] arrays, pcMax, pcArg, dcpaMin, dcpaArg [G] and
        `candidates` [G, 3] -- plus `ids`, the targets' ids in track order, and `best`: the index of the candidate with the smallest
        pcMax, then the largest dcpaMin, then the lowest index (evaluation.trial_best, on the host; None where no candidate has a pcMax).
        No live track: empty [G, 0] arrays, no device call, best None."""
        from . import evaluation
        for name, v in (("horizon", horizon), ("radius", radius), ("turnRate", turnRate)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
                raise ValueError("getTrialManoeuvres: %s must be a finite positive number (got %r)" % (name, v))
        if isinstance(delay, bool) or not isinstance(delay, (int, float, np.integer, np.floating)) or not np.isfinite(delay) or delay < 0:
            raise ValueError("getTrialManoeuvres: delay must be a finite number >= 0 (got %r)" % (delay,))
        if steps is None:
            steps = min(int(np.ceil(float(horizon) / float(self.radarPeriod))), evaluation.ENCOUNTER_MAX_STEPS)
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= evaluation.ENCOUNTER_MAX_STEPS:
            raise ValueError("getTrialManoeuvres: steps is an integer in 1 .. %d (got %r)" % (evaluation.ENCOUNTER_MAX_STEPS, steps))
        steps = int(steps)
        dt = float(horizon) / steps
        nx, Phi, Q = evaluation.encounter_model(self._model_mod, dt)
        own = np.asarray(ownShip, dtype=np.float64).reshape(-1)
        if len(own) != 4:
            raise ValueError("getTrialManoeuvres: ownShip is [x, y, vx, vy] (got %d components)" % len(own))
        dpsi, fs = np.asarray(courseChanges, dtype=np.float64).reshape(-1), np.asarray(speedFactors, dtype=np.float64).reshape(-1)
        if len(dpsi) == 0 or len(fs) == 0:
            raise ValueError("getTrialManoeuvres: courseChanges and speedFactors need one value at least")
        try:
            cand = evaluation.trial_candidates([(a, f, float(delay)) for a in dpsi for f in fs])
        except ValueError as exc:
            raise ValueError("getTrialManoeuvres: " + str(exc))
        x, P, ids = [], [], []
        nodes = list(self.__trackNodes__)
        if nodes:
            from . import smoothing
            chains = [smoothing.chain_inputs(node, self._model_mod.P0)[0] for node in nodes]
            ids += [leaf.ID if leaf.ID is not None else ch[0].ID if ch[0].ID is not None else -(i + 1) for i, (leaf, ch) in enumerate(zip(nodes, chains))]
            for xf, Pf in self.getFilteredTracks():
                x.append(np.asarray(xf, dtype=np.float64)[-1])
                P.append(np.asarray(Pf, dtype=np.float64)[-1])
        try:
            out = evaluation.trial_manoeuvres(np.array(x).reshape(len(x), nx), np.array(P).reshape(len(x), nx, nx), Phi, Q, steps, dt, float(radius), own, cand,
                                              float(turnRate), ownCovariance=ownCovariance, ctx=self._ctx)
        except ValueError as exc:
            raise ValueError("getTrialManoeuvres: " + str(exc))
        out["ids"] = ids
        out["best"] = evaluation.trial_best(out["pcMax"], out["dcpaMin"])
        return out

    @staticmethod
    def _selected_leaves(snap, nodes):
        """Per live track node the index of its leaf in leafBatch()'s arrays, or -1: the leaf of the node's target whose node is the track
        node's (a target born since the last scan is its own only leaf).  THE selection rule of getHypothesisEncounters,
        getGlobalHypotheses and getMonteCarloEncounters."""
        sel = np.full(len(nodes), -1, dtype=np.int64)
        for t, nd in enumerate(nodes):
            own_leaves = snap["target"] == t
            if nd._node < 0:      # (born after the last scan: the track node is the root itself, the target's only leaf)
                hit = np.flatnonzero(own_leaves) if own_leaves.sum() == 1 else ()
            else:
                hit = np.flatnonzero(own_leaves & (snap["node"] == nd._node))
            if len(hit):
                sel[t] = hit[0]
        return sel

    def getHypothesisEncounters(self, horizon, radius, ownShip, courseChanges=(0.0,), turnRate=None, speedFactors=(1.0,), delay=0.0, ownCovariance=None,
                                steps=None, leafTable=False):
        """getTrialManoeuvres held against EVERY LIVE HYPOTHESIS of every target, not only the selected one.  This is a multi-hypothesis
        tracker: per target the forest keeps the alternatives "that plot was clutter" and "it took the other plot", each with a state, a
        covariance and a cumulative score.  getEncounters and getTrialManoeuvres report the selected hypothesis alone; a second leaf of
        the same target, nearly as likely, may give a very different pc, and this is where it shows
        (evaluation.trial_hypotheses defines the figures).  Times count from the current scan.

        horizon, radius, ownShip, speedFactors, delay, ownCovariance, steps   as for getTrialManoeuvres
        courseChanges  as for getTrialManoeuvres; the default (0.0,) is "the own ship standing on"
        turnRate       the own ship's turn rate in rad/s, > 0.  Not needed while every course change is 0; required (ValueError) as soon
                       as one is not
        leafTable      True: the five [G, L] tables of the cells (candidate, leaf) are returned too
        The entries are leafBatch()'s leaves at the current scan: the forest's OWN states and covariances, nothing is re-filtered and no
        history is walked.  For an AIS-aided tracker they include the AIS updates (float64 covariances): the AIS gap of getEncounters
        and getTrialManoeuvres is closed for this output.  The selected leaf of a target is the one whose node is the live track node's
        (a target born since the last scan is its own only leaf).
        The hypothesis weights normalise INSIDE ONE TARGET, exp(-(cnllr - the target's smallest cnllr)); the exclusion constraints between
        targets, which the ILP enforces, are ignored -- the usual track-oriented approximation, not global-hypothesis probabilities.  The
        own ship and the leaves are taken as independent.  A constant-turn tracker raises NotImplementedError (model "ct": its transition
        depends on the state).
        Returns evaluation.trial_hypotheses' dict -- pcWorst, pcWorstLeaf, dcpaMin, dcpaMinLeaf, pcMean, pcSel, dcpaSel, tcpaSel [G, T],
        weight [L], nLeaves [T], candidates [G, 3] -- plus `ids` (the targets' ids in target order), `leafIds` (the target id of every
        leaf), and per candidate, folded over the targets on the host: `pcMeanMax` with `pcMeanMaxTarget`, `pcWorstMax` with
        `pcWorstMaxTarget` and `dcpaMinAll` with `dcpaMinAllTarget` [G] (NaN and -1 without a figure); `best`, evaluation.trial_best of
        (pcMeanMax, dcpaMinAll), and `bestWorstCase`, the same on pcWorstMax.  No live track: empty [G, 0] arrays, no device call."""
        from . import evaluation
        for name, v in (("horizon", horizon), ("radius", radius)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
                raise ValueError("getHypothesisEncounters: %s must be a finite positive number (got %r)" % (name, v))
        if isinstance(delay, bool) or not isinstance(delay, (int, float, np.integer, np.floating)) or not np.isfinite(delay) or delay < 0:
            raise ValueError("getHypothesisEncounters: delay must be a finite number >= 0 (got %r)" % (delay,))
        if steps is None:
            steps = min(int(np.ceil(float(horizon) / float(self.radarPeriod))), evaluation.ENCOUNTER_MAX_STEPS)
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= evaluation.ENCOUNTER_MAX_STEPS:
            raise ValueError("getHypothesisEncounters: steps is an integer in 1 .. %d (got %r)" % (evaluation.ENCOUNTER_MAX_STEPS, steps))
        steps = int(steps)
        dt = float(horizon) / steps
        nx, Phi, Q = evaluation.encounter_model(self._model_mod, dt)
        own = np.asarray(ownShip, dtype=np.float64).reshape(-1)
        if len(own) != 4:
            raise ValueError("getHypothesisEncounters: ownShip is [x, y, vx, vy] (got %d components)" % len(own))
        dpsi, fs = np.asarray(courseChanges, dtype=np.float64).reshape(-1), np.asarray(speedFactors, dtype=np.float64).reshape(-1)
        if len(dpsi) == 0 or len(fs) == 0:
            raise ValueError("getHypothesisEncounters: courseChanges and speedFactors need one value at least")
        if turnRate is None:
            if np.any(dpsi != 0):
                raise ValueError("getHypothesisEncounters: turnRate is required with a course change that is not 0")
            turnRate = 1.0      # (no candidate turns: the rate enters no figure)
        try:
            cand = evaluation.trial_candidates([(a, f, float(delay)) for a in dpsi for f in fs])
        except ValueError as exc:
            raise ValueError("getHypothesisEncounters: " + str(exc))
        nodes = list(self.__trackNodes__)
        T = len(nodes)
        ids = [int(i) for i in self._tbl_["id"]]
        if T:
            snap = self.leafBatch()
            sel = self._selected_leaves(snap, nodes)
            x, P, cn, tg, leaf_ids = snap["x"], np.asarray(snap["P"], dtype=np.float64), snap["cnllr"], snap["target"], snap["ID"].astype(np.int64)
        else:
            x, P, cn, tg, sel, leaf_ids = np.zeros((0, nx)), np.zeros((0, nx, nx)), np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        try:
            out = evaluation.trial_hypotheses(x, P, cn, tg, Phi, Q, steps, dt, float(radius), own, cand, turnRate, selected=sel, ownCovariance=ownCovariance,
                                              leafTable=leafTable, ctx=self._ctx)
        except ValueError as exc:
            raise ValueError("getHypothesisEncounters: " + str(exc))
        out["ids"], out["leafIds"] = ids, leaf_ids
        G = len(cand)
        for name, src, largest in (("pcMeanMax", "pcMean", True), ("pcWorstMax", "pcWorst", True), ("dcpaMinAll", "dcpaMin", False)):
            val, arg = np.full(G, np.nan), np.full(G, -1, dtype=np.int64)
            for g in range(G):
                row = out[src][g]
                if not np.isnan(row).all():
                    val[g] = np.nanmax(row) if largest else np.nanmin(row)
                    arg[g] = int(np.flatnonzero(row == val[g])[0])
            out[name], out[name + "Target"] = val, arg
        out["best"] = evaluation.trial_best(out["pcMeanMax"], out["dcpaMinAll"])
        out["bestWorstCase"] = evaluation.trial_best(out["pcWorstMax"], out["dcpaMinAll"])
        return out

    def _mc_leaves(self, name, nx, hypotheses, weights):
        """The leaves and weights of a Monte-Carlo call, gathered once for getMonteCarloEncounters and getMonteCarloPairEncounters:
        leafBatch()'s leaves (the AIS-updated float64 ones of an AIS-aided tracker) with exp(-(cnllr - the target's smallest cnllr)) or
        the caller's `weights`; hypotheses=False: the selected leaf of every target alone.  (x, P, target, leafIds, weight, ids)."""
        nodes = list(self.__trackNodes__)
        ids = [int(i) for i in self._tbl_["id"]]
        if nodes:
            snap = self.leafBatch()
            x, P, tg, leaf_ids = snap["x"], np.asarray(snap["P"], dtype=np.float64), np.asarray(snap["target"]), snap["ID"].astype(np.int64)
            if weights is not None:
                w = np.asarray(weights, dtype=np.float64)
                if w.shape != (len(x),):
                    raise ValueError("%s: weights is an [L] = [%d] array, one per leaf of leafBatch() (got shape %r)" % (name, len(x), w.shape))
                if np.isnan(w).any():
                    t = int(tg[np.flatnonzero(np.isnan(w))[0]])
                    raise ValueError("%s: a weight of target %d (id %s) is NaN" % (name, t, ids[t] if t < len(ids) else "?"))
            else:
                cn = np.asarray(snap["cnllr"], dtype=np.float64)
                w = np.zeros(len(x))
                for t in np.unique(tg):
                    at = np.flatnonzero(tg == t)
                    if not np.isnan(cn[at]).all():
                        with np.errstate(all="ignore"):
                            w[at] = np.where(np.isnan(cn[at]), 0.0, np.exp(-(cn[at] - np.nanmin(cn[at]))))
            if not hypotheses:
                sel = self._selected_leaves(snap, nodes)
                sel = sel[sel >= 0]
                x, P, tg, leaf_ids, w = x[sel], P[sel], tg[sel], leaf_ids[sel], np.ones(len(sel))
        else:
            x, P, tg, leaf_ids, w = np.zeros((0, nx)), np.zeros((0, nx, nx)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0)
        return x, P, tg, leaf_ids, w, ids

    def _mc_horizon(self, name, horizon, radius, steps):
        """What both getMonteCarlo* calls make of (horizon, radius, steps), ValueError under the caller's `name`: (steps, dt, nx, Phi, Q,
        ct) -- the steps (None: one per radar period, at most evaluation.ENCOUNTER_MAX_STEPS), dt = horizon / steps, and the model's
        matrices of one step, widened from float32; ct: a constant-turn tracker, whose Phi no particle reads."""
        from . import evaluation
        for what, v in (("horizon", horizon), ("radius", radius)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
                raise ValueError("%s: %s must be a finite positive number (got %r)" % (name, what, v))
        if steps is None:
            steps = min(int(np.ceil(float(horizon) / float(self.radarPeriod))), evaluation.ENCOUNTER_MAX_STEPS)
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= evaluation.ENCOUNTER_MAX_STEPS:
            raise ValueError("%s: steps is an integer in 1 .. %d (got %r)" % (name, evaluation.ENCOUNTER_MAX_STEPS, steps))
        steps = int(steps)
        dt = float(horizon) / steps
        model = self._model_mod
        ct = getattr(model, "transition", None) == "ct"
        if ct:
            nx = 6
            widen = lambda m: np.ascontiguousarray(np.asarray(m, dtype=np.float32).astype(np.float64).reshape(nx, nx))
            Phi, Q = widen(model.Phi(dt, 0.0)), widen(model.Q(dt))      # (Phi is not read: every particle has its own)
        else:
            nx, Phi, Q = evaluation.encounter_model(model, dt)
        return steps, dt, nx, Phi, Q, ct

    def _mc_candidates(self, name, horizon, radius, steps, ownShip, courseChanges, turnRate, speedFactors, delay, make):
        """The candidate handling getMonteCarloEncounters and getMonteCarloDomainEncounters share, ValueError under the caller's `name`:
        the delay, `_mc_horizon`, the own ship, the candidates (every course change with every speed factor, at most 64, none NaN) and
        what `make` (evaluation.mc_own_paths or evaluation.mc_own_poses) makes of them.  (steps, dt, nx, Phi, Q, ct, cand [G, 3], made)."""
        from . import evaluation
        if isinstance(delay, bool) or not isinstance(delay, (int, float, np.integer, np.floating)) or not np.isfinite(delay) or delay < 0:
            raise ValueError("%s: delay must be a finite number >= 0 (got %r)" % (name, delay))
        steps, dt, nx, Phi, Q, ct = self._mc_horizon(name, horizon, radius, steps)
        own = np.asarray(ownShip, dtype=np.float64).reshape(-1)
        if len(own) != 4 or not np.isfinite(own).all():
            raise ValueError("%s: ownShip is a finite [x, y, vx, vy] (got %r)" % (name, ownShip))
        dpsi, fs = np.asarray(courseChanges, dtype=np.float64).reshape(-1), np.asarray(speedFactors, dtype=np.float64).reshape(-1)
        if len(dpsi) == 0 or len(fs) == 0:
            raise ValueError("%s: courseChanges and speedFactors need one value at least" % name)
        if turnRate is None:
            if np.any(dpsi != 0):
                raise ValueError("%s: turnRate is required with a course change that is not 0" % name)
            turnRate = 1.0      # (no candidate turns: the rate enters no figure)
        try:
            cand = evaluation.trial_candidates([(a, f, float(delay)) for a in dpsi for f in fs])
            if len(cand) > evaluation.MC_MAX_PATHS or np.isnan(cand).any():
                raise ValueError("at most %d candidates, none of them NaN (got %d)" % (evaluation.MC_MAX_PATHS, len(cand)))
            made = make(own, cand, turnRate, steps, dt)
        except ValueError as exc:
            raise ValueError("%s: %s" % (name, exc))
        return steps, dt, nx, Phi, Q, ct, cand, made

    def getMonteCarloEncounters(self, horizon, radius, ownShip, particles=4096, seed=0, courseChanges=(0.0,), turnRate=None, speedFactors=(1.0,), delay=0.0,
                                steps=None, hypotheses=True, weights=None):
        """Encounters by MONTE CARLO (evaluation.mc_encounters defines the figures): particles drawn from the forest's own leaves -- a
        Gaussian mixture per target --, walked with the model's process noise and held against the own ship's candidate paths.  It gives
        what getEncounters, getTrialManoeuvres and getHypothesisEncounters cannot: `pEver`, the probability of coming within `radius` AT
        ANY TIME of the horizon (their pc is the largest per-step mass); a target whose leaves disagree sampled as the mixture it is
        (their pcMean averages Gaussian cells); and CONSTANT-TURN trackers (models/ct), which those three refuse -- here every particle
        turns at its own rate, Phi(dt, w) of the real model.  Works for models/pv, models/ca and models/ct.  Times count from the
        current scan.

        horizon, radius, ownShip, courseChanges, turnRate, speedFactors, delay, steps   as for getHypothesisEncounters; at most 64
                       candidates
        particles, seed   particles per target (a multiple of 64 in 64 .. 2^20) and the seed: one seed, one result, bit for bit
        hypotheses     True: every leaf of leafBatch() with the weight exp(-(cnllr - the target's smallest cnllr)) inside its target (a
                       leaf without a cnllr, or with +inf: weight 0).  False: the selected leaf of every target alone, by
                       getHypothesisEncounters' selection rule (a target without one is left out)
        weights        None, or [L]: replaces those weights, e.g. getGlobalHypotheses()['leafProbability'] -- through it the exclusion
                       constraints between targets reach an encounter figure.  A NaN in it raises ValueError and names the target
        The entries are leafBatch()'s leaves at the current scan, the forest's OWN states: nothing is re-filtered.  For an AIS-aided
        tracker they are the AIS-updated float64 ones.  The own ship is a path without a covariance; targets are independent of each
        other.  Pairs of targets: getMonteCarloPairEncounters.
        Returns evaluation.mc_encounters' dict -- within, ever, valid, status, pc, pcMax, tpc, pEver, sePcMax, sePEver, targets, first,
        cdf, order -- plus `ids` (the id of every target of the result, in its order), `leafIds` (the target id of every leaf used),
        `candidates` [G, 3], and per candidate `pEverMax` with `pEverMaxTarget` (the largest pEver over the targets and its index into
        the result's targets; NaN and -1 without a figure) and `best`: the candidate with the smallest pEverMax, among equal ones the
        LOWEST INDEX (evaluation.trial_best with every dcpa equal: a Monte-Carlo run has no dcpa to break a tie with); None if no
        candidate has a figure.  No live track: empty arrays, no device call."""
        from . import evaluation
        name = "getMonteCarloEncounters"
        steps, dt, nx, Phi, Q, ct, cand, paths = self._mc_candidates(name, horizon, radius, steps, ownShip, courseChanges, turnRate, speedFactors, delay,
                                                                     evaluation.mc_own_paths)
        x, P, tg, leaf_ids, w, ids = self._mc_leaves(name, nx, hypotheses, weights)
        try:
            out = evaluation.mc_encounters(x, P, tg, w, Phi, Q, steps, dt, float(radius), paths, particles=particles, seed=seed,
                                           transition="ct" if ct else "linear", ctx=self._ctx)
        except ValueError as exc:
            raise ValueError("%s: %s" % (name, exc))
        out["ids"] = [ids[t] if t < len(ids) else -1 for t in out["targets"]]
        out["leafIds"], out["candidates"] = leaf_ids, cand
        G = len(cand)
        val, arg = np.full(G, np.nan), np.full(G, -1, dtype=np.int64)
        for g in range(G):
            row = out["pEver"][g]
            if len(row) and not np.isnan(row).all():
                val[g] = np.nanmax(row)
                arg[g] = int(np.flatnonzero(row == val[g])[0])
        out["pEverMax"], out["pEverMaxTarget"] = val, arg
        out["best"] = evaluation.trial_best(val, np.zeros(G))
        return out

    def getMonteCarloPairEncounters(self, horizon, radius, particles=4096, seed=0, steps=None, pairs=None, screen=None, hypotheses=True, weights=None):
        """Encounters by MONTE CARLO between PAIRS OF TARGETS (evaluation.mc_pair_encounters defines the figures): target against target,
        what a VTS operator or a fleet monitor asks for, with the engine of getMonteCarloEncounters -- particles drawn from the forest's
        own leaves, a Gaussian mixture per target, walked with the model's process noise; particle p of one target is held against
        particle p of the other.  Next to `pEver` it gives `firstAt` and `pEverBy`, the distribution of the time to the first violation.
        getEncounters(ownShip=None) is the Gaussian rule for the same question: one re-filtered Gaussian per track, the largest per-step
        mass, and no constant-turn tracker.  Works for models/pv, models/ca and models/ct.  Times count from the current scan.

        horizon, radius, particles, seed, steps, hypotheses, weights   as for getMonteCarloEncounters
        pairs          [n, 2] pairs of target INDICES (leafBatch()'s `target`, the order of getTrackNodes()), or None
        screen         with pairs=None: the `distance` of evaluation.mc_pair_screen over `horizon` -- only pairs whose straight-line
                       closest approach is below it are scored.  A PRE-FILTER: a pair it drops gets no result; choose it generously,
                       more so for a constant-turn tracker
        With pairs and screen both None all T (T - 1) / 2 pairs are taken, if that is at most evaluation.MC_MAX_PAIRS = 2^20; beyond it
        ValueError asks for a screen.
        Returns evaluation.mc_pair_encounters' dict -- within, firstAt, ever, valid, status, pc, pcMax, tpc, pEver, sePcMax, sePEver,
        pEverBy, pairs, targets, first, cdf, order -- plus `ids` [n, 2] (the two target ids of every pair), `leafIds` (the target id of
        every leaf used), `ranking` (the pair indices by descending pEver, ties by index, pairs that are not scored last) and `worst`
        (ranking[0], or None without a pair).  Fewer than two live targets: empty arrays, no device call.
        Out of scope: correlation between targets, the own ship's covariance (there is no own ship here), pairs across
        getHypothesisEncounters' Gaussian cells, and firstAt for getMonteCarloEncounters."""
        from . import evaluation
        name = "getMonteCarloPairEncounters"
        steps, dt, nx, Phi, Q, ct = self._mc_horizon(name, horizon, radius, steps)
        x, P, tg, leaf_ids, w, ids = self._mc_leaves(name, nx, hypotheses, weights)
        present = np.unique(tg)
        try:
            if len(present) < 2:
                if pairs is not None and np.size(pairs):
                    raise ValueError("pairs were given, and fewer than two targets are live")
                pairs = np.zeros((0, 2), dtype=np.int64)
            elif pairs is None and screen is not None:
                pairs = evaluation.mc_pair_screen(x, tg, w, float(horizon), screen)
            elif pairs is None:
                T = len(present)
                if T * (T - 1) // 2 > evaluation.MC_MAX_PAIRS:
                    raise ValueError("%d targets make %d pairs, more than %d: give screen= (or pairs=)" % (T, T * (T - 1) // 2, evaluation.MC_MAX_PAIRS))
                a, b = np.triu_indices(T, 1)
                pairs = np.stack([present[a], present[b]], axis=1).astype(np.int64)
            if len(present) < 2:      # (no pair: nothing is uploaded)
                x, P, tg, leaf_ids, w = x[:0], P[:0], tg[:0], leaf_ids[:0], w[:0]
            out = evaluation.mc_pair_encounters(x, P, tg, w, Phi, Q, steps, dt, float(radius), pairs, particles=particles, seed=seed,
                                                transition="ct" if ct else "linear", ctx=self._ctx)
        except ValueError as exc:
            raise ValueError("%s: %s" % (name, str(exc).replace("mc_pair_screen: distance", "mc_pair_screen: screen", 1)))
        lookup = lambda t: ids[t] if 0 <= t < len(ids) else -1
        out["ids"] = np.array([[lookup(int(a)), lookup(int(b))] for a, b in out["pairs"]], dtype=np.int64).reshape(-1, 2)
        out["leafIds"] = leaf_ids
        p = out["pEver"]
        n = len(p)
        out["ranking"] = np.lexsort((np.arange(n), np.where(np.isnan(p), np.inf, -p))).astype(np.int64)
        out["worst"] = int(out["ranking"][0]) if n else None
        return out

    def getMonteCarloZoneEncounters(self, horizon, zones, particles=4096, seed=0, steps=None, hypotheses=True, weights=None):
        """GUARD ZONES by MONTE CARLO (evaluation.mc_zone_encounters defines the figures): will a target enter a PLACE -- a restricted
        area, a shoal contour, an anchorage, a traffic-separation zone --, with what probability within `horizon`, and when.  The other
        forward-looking outputs measure a target against something that moves (the own ship, another target); this one measures it
        against polygons that stand still, with the engine of getMonteCarloEncounters -- particles drawn from the forest's own leaves, a
        Gaussian mixture per target, walked with the model's process noise, the same particles for the same seed.  A zone thinner than
        one step's travel is not stepped over: the path between two steps is held against the zone's edges.  Works for models/pv,
        models/ca and models/ct, and for AIS-aided trackers.  Times count from the current scan.

        horizon, particles, seed, steps, hypotheses, weights   as for getMonteCarloEncounters
        zones          a list of [V, 2] arrays: the vertices of every zone in metres, the tracker's frame; at most 32 zones of 3
                       vertices at least, 1 024 vertices in all; either orientation, concave polygons included
        Returns evaluation.mc_zone_encounters' dict -- inside, firstAt, ever, valid, status, pInside, pInsideMax, tInside, pEver,
        pEverBy, sePInsideMax, sePEver, zoneFirst, zoneXY, targets, first, cdf, order -- plus `ids` (the id of every target of the
        result, in its order), `leafIds` (the target id of every leaf used) and `ranking` [n, 2]: the (zone, target) cells by
        descending pEver, ties by zone and then target, cells without a figure last.  No live target or no zone: empty arrays, no
        device call.
        Zones that move with the own ship (a polygonal ship domain) are getMonteCarloDomainEncounters' case.  Out of scope: open gates
        and polylines (a thin quadrilateral serves), holes, geodetic coordinates, the dwell time inside a zone."""
        from . import evaluation
        name = "getMonteCarloZoneEncounters"
        steps, dt, nx, Phi, Q, ct = self._mc_horizon(name, horizon, 1.0, steps)
        try:
            evaluation.mc_zone_pack(zones, name)      # (before the leaves are gathered: a zone that does not fit costs no device read)
            if len(zones) == 0:      # (no zone: no leaf is read and nothing is uploaded)
                x, P, tg, leaf_ids, w, ids = np.zeros((0, nx)), np.zeros((0, nx, nx)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0), []
            else:
                x, P, tg, leaf_ids, w, ids = self._mc_leaves(name, nx, hypotheses, weights)
            out = evaluation.mc_zone_encounters(x, P, tg, w, Phi, Q, steps, dt, zones, particles=particles, seed=seed, transition="ct" if ct else "linear",
                                                ctx=self._ctx)
        except ValueError as exc:
            text = str(exc)
            raise ValueError(text if text.startswith(name) else "%s: %s" % (name, text))
        out["ids"] = [ids[t] if t < len(ids) else -1 for t in out["targets"]]
        out["leafIds"] = leaf_ids
        p = out["pEver"]
        Z, T = p.shape
        zz, tt = np.divmod(np.arange(Z * T), max(T, 1))
        flat = p.reshape(-1)
        order = np.lexsort((np.arange(Z * T), np.where(np.isnan(flat), np.inf, -flat)))
        out["ranking"] = np.stack([zz[order], tt[order]], axis=1).astype(np.int64).reshape(-1, 2)
        return out

    def getMonteCarloDomainEncounters(self, horizon, domains, ownShip, particles=4096, seed=0, courseChanges=(0.0,), turnRate=None, speedFactors=(1.0,), delay=0.0,
                                      steps=None, hypotheses=True, weights=None):
        """SHIP DOMAINS by MONTE CARLO (evaluation.mc_domain_encounters defines the figures): will a target enter the safety region
        AROUND THE OWN SHIP -- a polygon in the ship's body frame, longer ahead than astern and usually wider to starboard than to port,
        carried along and turned with every candidate path --, with what probability within `horizon`, and when.  The disc of
        getMonteCarloEncounters cannot tell a target that passes astern from one that passes ahead; the zones of
        getMonteCarloZoneEncounters stand still.  The engine is theirs: particles drawn from the forest's own leaves, a Gaussian mixture
        per target, walked with the model's process noise, the same particles for the same seed.  Works for models/pv, models/ca and
        models/ct.  Times count from the current scan.

        horizon, ownShip, courseChanges, turnRate, speedFactors, delay, steps, particles, seed, hypotheses, weights   as for
                       getMonteCarloEncounters; the own ship must move (a ship of speed 0 has no heading: ValueError)
        domains        a list of 1 .. 4 [V, 2] arrays: the vertices of every domain in metres IN THE BODY FRAME, the first coordinate to
                       the right of the heading and the second ahead (drawn bow-up), 3 vertices each at least, 256 in all at most;
                       (domains) x (candidates) <= 64 cells.  THE DECIDING DOMAIN GOES FIRST: `best` looks at domain 0 alone (an inner
                       "collision" domain first, an outer "comfort" domain behind it)
        The body-frame path between two steps is taken as STRAIGHT: on a step inside a turn of the own ship it is a chord of a curved
        path (shorter steps are the remedy).
        Returns evaluation.mc_domain_encounters' dict -- inside, firstAt, ever, valid, status, pInside, pInsideMax, tInside, pEver,
        pEverBy, sePInsideMax, sePEver, domFirst, domXY, ownPoses, targets, first, cdf, order -- plus `ids` (the id of every target of
        the result, in its order), `leafIds` (the target id of every leaf used), `candidates` [G, 3], per (domain, candidate) `pEverMax`
        [nDomain, G] with `pEverMaxTarget` (the largest pEver over the targets and its index into the result's targets; NaN and -1
        without a figure) and `best`: the candidate with the smallest pEverMax of DOMAIN 0, among equal ones the lowest index; None if
        no candidate has a figure.  No live track: empty arrays, no device call.
        Out of scope: domains around targets or between pairs of targets, a domain that scales with speed, the own ship's covariance,
        a curved body-frame path inside a turning step, holes, more than 64 cells, a stationary own ship."""
        from . import evaluation
        name = "getMonteCarloDomainEncounters"
        steps, dt, nx, Phi, Q, ct, cand, poses = self._mc_candidates(name, horizon, 1.0, steps, ownShip, courseChanges, turnRate, speedFactors, delay,
                                                                     evaluation.mc_own_poses)
        try:
            df, _ = evaluation.mc_domain_pack(domains, name)      # (before the leaves are gathered: a domain that does not fit costs no device read)
            if (len(df) - 1) * len(cand) > evaluation.MC_DOMAIN_MAX_CELLS:
                raise ValueError("%s: at most %d cells, (domains) x (candidates) (got %d x %d)" % (name, evaluation.MC_DOMAIN_MAX_CELLS, len(df) - 1, len(cand)))
            x, P, tg, leaf_ids, w, ids = self._mc_leaves(name, nx, hypotheses, weights)
            out = evaluation.mc_domain_encounters(x, P, tg, w, Phi, Q, steps, dt, domains, poses, particles=particles, seed=seed,
                                                  transition="ct" if ct else "linear", ctx=self._ctx)
        except ValueError as exc:
            text = str(exc)
            raise ValueError(text if text.startswith(name) else "%s: %s" % (name, text))
        out["ids"] = [ids[t] if t < len(ids) else -1 for t in out["targets"]]
        out["leafIds"], out["candidates"] = leaf_ids, cand
        D, G = out["pEver"].shape[:2]
        val, arg = np.full((D, G), np.nan), np.full((D, G), -1, dtype=np.int64)
        for d in range(D):
            for g in range(G):
                row = out["pEver"][d, g]
                if len(row) and not np.isnan(row).all():
                    val[d, g] = np.nanmax(row)
                    arg[d, g] = int(np.flatnonzero(row == val[d, g])[0])
        out["pEverMax"], out["pEverMaxTarget"] = val, arg
        out["best"] = evaluation.trial_best(val[0], np.zeros(G))
        return out

    def leafRows(self):
        """The keys of the plots on every current leaf's window path, [L, N + 1] int32 in leafBatch() order (`mht_forest_leaf_rows`): per
        ancestor with a measurement, from the leaf up to its target's window root (the root itself only where it is the leaf),
        (level << 24) | measurement number with level = scans back from the current one; -1 elsewhere.  Two leaves share a key exactly
        where the ILP lets only one of them be selected.  aisAided=True raises NotImplementedError (its columns carry message rows too)."""
        if self._ais:
            raise NotImplementedError("leafRows: not for an aisAided tracker -- its ILP columns also carry AIS message rows")
        snap = self._leaf_snapshot()
        L, depth = len(snap["node"]), int(self._cfg.n_scan) + 1
        rows = np.full((max(L, 1), depth), -1, dtype=np.int32)
        n = C.c_int32(0)
        _lib.check(self._lib.mht_forest_leaf_rows(self._ctx.handle, L, depth, rows.ctypes.data_as(C.c_void_p), C.byref(n)))
        if n.value != L:
            raise RuntimeError("leafRows: the forest has %d leaves, leafBatch() had %d" % (n.value, L))
        return rows[:L]

    def getGlobalHypotheses(self, k=8, nodeLimit=1 << 20):
        """The k best GLOBAL hypotheses of every cluster of the current leaves: the joint answers -- one leaf per target, no plot used
        twice -- ranked by their summed cnllr, where getHypothesisEncounters' weights look at one target at a time.  It answers how
        ambiguous a cluster is, what the second-best joint explanation is, and how probable a leaf is once the other targets have had
        their say (evaluation.k_best_hypotheses defines the figures and the search; cost = cnllr, so prob is proportional to
        exp(-sum cnllr)).  Works for 4-state, 6-state and constant-turn trackers alike: the search is model-free.

        THE LIST IS OVER THE CURRENT LEAVES, AFTER PRUNING: what the last scan's N-scan pruning removed is gone, and a target terminated
        in the last scan has freed its plots -- so rank 0 may be CHEAPER than the tracker's own selection, which was made with that
        target still competing.  prob and leafProbability are TRUNCATED to the k listed hypotheses (they sum to 1 over the list, not over
        all global hypotheses).  Clusters that were not searched (status 2 or 3: beyond 32 targets, 1024 leaves or 2048 plots) are
        flagged, not guessed.  The clusters are the connected components of targets whose leaves share a plot inside the window: finer
        than the scan's gating clusters.
        A target born since the last scan is its own only leaf and takes part with NO key: the number of its plot counts the scan's
        unused plots (the initiator's numbering, as in the reference), so it says nothing about the plots of the other leaves, and the
        reference's own ILP never sees it either (a window root is left out of its rows).
        Returns evaluation.k_best_hypotheses' dict -- clusters, count, status, nodes [C], cost, prob [C, k], selection [k, T],
        leafProbability [L] -- plus `rows` [L, N + 1] (the keys the search used: leafRows() with those targets' blanked), `ids` (the targets' ids in target order), `leafIds` (the target id of every leaf), `selected` [T]
        (the leaf of each live track node, found as getHypothesisEncounters finds it; -1 if none) and `selectedRank` [C]: the rank of the
        tracker's own selection in its cluster's list, or -1 where it is not among the k listed.  No live track: empty arrays, no device
        call.  aisAided=True raises NotImplementedError."""
        from . import evaluation
        if self._ais:
            raise NotImplementedError("getGlobalHypotheses: not for an aisAided tracker -- its ILP columns also carry AIS message rows")
        nodes = list(self.__trackNodes__)
        T = len(nodes)
        ids = [int(i) for i in self._tbl_["id"]]
        if T == 0:
            out = evaluation.k_best_hypotheses(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros((0, 1), dtype=np.int32), k, nodeLimit)
            out.update(rows=np.zeros((0, int(self._cfg.n_scan) + 1), dtype=np.int32), ids=ids, leafIds=np.zeros(0, dtype=np.int64),
                       selected=np.zeros(0, dtype=np.int64), selectedRank=np.zeros(0, dtype=np.int64))
            return out
        snap = self.leafBatch()
        rows = self.leafRows().copy()
        born = np.array([nd._node < 0 for nd in nodes], dtype=bool)
        if born.any():      # (see the docstring: such a leaf's key is in the initiator's numbering)
            tg = snap["target"]
            rows[born[np.minimum(tg, T - 1)] & (tg < T)] = -1
        out = evaluation.k_best_hypotheses(snap["cnllr"], snap["target"], rows, k, nodeLimit, ctx=self._ctx)
        out["rows"] = rows
        sel = self._selected_leaves(snap, nodes)
        rank = np.full(len(out["clusters"]), -1, dtype=np.int64)
        for c, tg in enumerate(out["clusters"]):
            tg = tg[tg < T]
            for r in range(int(out["count"][c])):
                if len(tg) and (out["selection"][r, tg] == sel[tg]).all():
                    rank[c] = r
                    break
        out.update(ids=ids, leafIds=snap["ID"].astype(np.int64), selected=sel, selectedRank=rank)
        return out

    def getOspa2(self, truth, c, p=2, window=None, every=1, terminated=True, smooth=False, constantTurn=False, ais=False, truthIds=None):
        """The track histories scored against the truth TRAJECTORIES: OSPA(2) over windows of steps (evaluation.ospa2_windows, which
        defines the figures).  Per-scan GOSPA assigns every scan on its own, so this is the figure that sees whether the targets were
        KEPT: a track cut into fragments, two tracks that swap targets and a late confirmation all cost here and score 0 there.

        truth      getGospa's two forms: a sequence of (time, positions [m, >= 2]), or a pair (times, positions per time)
        truthIds   None: a truth's identity is its row index, and every step needs the same number of rows (ValueError otherwise).  Else
                   per step the identities of the step's rows (any hashable, as evaluation.id_switches takes them).  A row whose first
                   two columns are NaN is absent at that step.
        c, p       the cut-off and the exponent (1 or 2)
        window, every   None: one window, the whole run; W: sliding windows of W steps that end at steps 0, every, 2 every, ...
        The steps are the truth's times.  A track is one history -- a node of __trackNodes__, with terminated=True (the default) also of
        __terminatedTargets__, and its ancestors -- present at the steps whose time one of its nodes carries (compared with == on the
        float the MeasurementList carried); nodes at other times, the initial state of a track among them, are left out and counted in
        nIgnored.  smooth, constantTurn and ais as in getGospa, with the same refusals.

        THESE ARE THE HISTORIES AS THEY STAND AT THE CALL: resolved by the N-scan window, every track one chain.  They are not the
        estimates the tracker reported online at each scan, which a hypothesis pruned since may have produced.

        Returns ospa2_windows' dict (ospa2, total, localisation, cardinality, nAssigned, nTracks, nTruths, windows, match [n_win, n]
        with the truth's COLUMN: its row index, or its place in order of first appearance under truthIds) plus times (of the windows'
        last steps), trackIds [n], nIgnored and meanOspa2 (NaN without windows)."""
        from . import evaluation
        if (constantTurn or ais) and not smooth:
            raise ValueError("getOspa2: constantTurn and ais select the smoother of smooth=True; the filtered positions need neither")
        c, p = evaluation._check_cutoff(c, p)
        times, Y = evaluation.truth_steps(truth)
        truthXY, truthOn = evaluation.truth_trajectories(Y, truthIds)
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        smoothed = self._smooth_nodes(nodes, constantTurn=constantTurn, ais=ais) if smooth else None
        step_of = {}
        for s, t in enumerate(times):
            step_of.setdefault(float(t), s)
        trackXY = np.full((len(times), len(nodes), 2), np.nan)
        trackOn = np.zeros((len(times), len(nodes)), dtype=np.uint8)
        ids, nIgnored = [], 0
        for i, leaf in enumerate(nodes):
            chain = leaf.backtrackNodes()
            ids.append(leaf.ID if leaf.ID is not None else chain[0].ID if chain[0].ID is not None else -(i + 1))
            for k, node in enumerate(chain):
                s = step_of.get(float(node.time))
                if s is None:
                    nIgnored += 1
                    continue
                pos = smoothed[i][0][k] if smooth and len(chain) >= 2 else node.x_0[0:2]      # (a chain of one node has nothing to smooth)
                trackXY[s, i] = np.asarray(pos, dtype=np.float64).reshape(2)
                trackOn[s, i] = 1
        out = evaluation.ospa2_windows(trackXY, trackOn, truthXY, truthOn, c, p, window=window, every=every, ctx=self._ctx)
        out["times"] = times[out["windows"][:, 1]] if len(out["windows"]) else np.zeros(0)
        out["trackIds"], out["nIgnored"] = ids, nIgnored
        out["meanOspa2"] = float(np.mean(out["ospa2"])) if len(out["ospa2"]) else float("nan")
        return out

    def getLikelihoodSurface(self, qScales, rScales, terminated=False, constantTurn=False):
        """getTrackLikelihoods under a grid of noise levels in ONE device call: candidate (iq, ir) scores the same tracks with
        qScales[iq] * Q(T) and rScales[ir] * R in place of the tracker's own (smoothing.noise_grid, score_nodes_grid; scales finite and
        positive, else ValueError).  The pooled maximum-likelihood (Q, R) over the grid for ALL tracks -- one pair the constructor can
        take, which per-track EM does not give -- and how flat the optimum is.  Returns a dict:
            qScales, rScales     the grid, float64
            ll, nis [nq, nr]     the tracks' log-likelihoods and NIS summed (np.sum in float64 on the host)
            nObs                 the plots scored, int (the same for every cell)
            trackLl, trackNis [nq, nr, n], trackNObs [n]     per track, in getTrackLikelihoods' order
            best                 (iq, ir) of the largest finite ll, the first on ties; None if no cell is finite
        Cell (iq, ir) with both scales 1 holds getTrackLikelihoods' figures bit for bit.  terminated and constantTurn as there, with
        the same refusals.  There is no ais switch: the messages of an AIS-aided tracker are NOT scored, its tracks are scored from
        their radar plots under the linear model."""
        from . import smoothing
        nodes = list(self.__trackNodes__)
        if terminated:
            nodes += list(self.__terminatedTargets__)
        Q, R = smoothing.noise_grid(self._model_mod, self.radarPeriod, qScales, rScales)
        q, r = np.asarray(qScales, dtype=np.float64).reshape(-1), np.asarray(rScales, dtype=np.float64).reshape(-1)
        ll, nis, nobs = smoothing.score_nodes_grid(self._model_mod, self.radarPeriod, nodes, Q, R, ctx=self._ctx, constantTurn=constantTurn)
        shape = (len(q), len(r), len(nodes))
        out = {"qScales": q, "rScales": r, "trackLl": ll.reshape(shape), "trackNis": nis.reshape(shape), "trackNObs": nobs,
               "nObs": int(nobs.sum())}
        out["ll"], out["nis"] = np.sum(out["trackLl"], axis=2), np.sum(out["trackNis"], axis=2)
        out["best"] = smoothing.best_cell(out["ll"])
        return out

    def synchronize(self):
        """Wait for everything queued on the device and fold it (reports are folded lazily otherwise)."""
        self._drain()
        self._ctx.synchronize()

    # ---- the reference's console log (tracker.py:129-137, :1402-1467): same columns, fed from the device's scan report ---------------
    def setHighPriority(self):
        import platform
        import psutil
        proc = psutil.Process()
        proc.nice(psutil.HIGH_PRIORITY_CLASS if platform.system() == "Windows" else 5)

    def getTimeLogHeader(self):
        cols = (('{:3} ', "Nr"), ('{:9} ', "Num Targets"), ('{:12} ', "Iteration (ms)"),
                ('({0:23} ', "(nMeasurements + nAisUpdates / nNodes) Process time ms"))
        return ("".join(f.format(v) for f, v in cols) + '({0:2}) {1:5}'.format("nClusters", 'Cluster') +
                '({0:3}) {1:6}'.format("nOptimSolved", 'Optim') + '{:4}'.format('DynN') + '{:5}'.format('N-Prune') +
                '{:3}'.format('Terminate') + '{:5}'.format('Init'))

    def getTimeLogString(self):
        """One line per scan like the reference's.  Stage times are the device's (with `deviceTiming=True`; otherwise only Total and
        Init are known); the node count of the reference's line is the number of hypotheses the scan produced (children of the grow
        kernel): the forest keeps no per-target node totals."""
        st = self.lastScanStats
        ms = {k: 1e3 * self.toc.get(k, 0.0) for k in ('Total', 'Process', 'Cluster', 'Optim', 'DynN', 'N-Prune', 'Terminate', 'Init')}
        return ('{:<3.0f} '.format(len(self.__scanHistory__)) + 'nTrack {:2.0f} '.format(len(self.__targetList__)) +
                'Total {0:6.0f} '.format(ms['Total']) +
                'Process({0:4.0f}+{1:<3.0f}/{2:6.0f}) {3:6.1f} '.format(st["M"], 0, st["L"] + st["G"], ms['Process']) +
                'Cluster({0:2.0f}) {1:5.1f} '.format(st["clusters"], ms['Cluster']) +
                'Optim({0:g}) {1:6.1f} '.format(self.nOptimSolved, ms['Optim']) + 'DynN {:4.1f} '.format(ms['DynN']) +
                'N-Prune {:5.1f} '.format(ms['N-Prune']) + 'Kill {:3.1f} '.format(ms['Terminate']) + 'Init {:5.1f}'.format(ms['Init']))

    def printTimeLog(self, **kwargs):
        late = self.toc['Total'] > self.radarPeriod
        print(("!! " if late else "   ") + self.getTimeLogString())      # (the reference colours the line with termcolor)

    def printTimeLogHeader(self):
        print(self.getTimeLogHeader())

    @staticmethod
    def printClusterList(clusterList):
        print("Clusters:")
        for i, cluster in enumerate(clusterList):
            print("Cluster ", i, " contains target(s):\t", cluster, sep="")

    def printTargetList(self, **kwargs):
        np.set_printoptions(precision=2, suppress=True)
        print("TargetList:")
        for i, target in enumerate(self.__targetList__):
            print("%3d: %s" % (i, target))
        print()

    # ---- XML result export (tracker.py:1469-1545): what the reference's evaluation scripts read ----------------------------------
    def getScenarioElement(self, **kwargs):
        import xml.etree.ElementTree as ET
        return ET.Element(xmltags.scenarioTag)

    def _storeTrackerArgs(self, scenarioElement, **kwargs):
        import xml.etree.ElementTree as ET
        for key, value in kwargs.items():
            scenarioElement.attrib[str(key)] = str(value)
        settings = ET.SubElement(scenarioElement, xmltags.trackerSettingsTag)
        for name, value in (("M_required", self.M_required), ("N_checks", self.N_checks), ("mergeThreshold", self.mergeThreshold),
                            ("ownPosition", self.position), ("radarRange", self.radarRange), ("radarPeriod", self.radarPeriod),
                            ("lambdaPhi", self.lambda_phi), ("lambdaNu", self.lambda_nu), ("lambdaEx", self.lambda_ex), ("eta2", self.eta2),
                            ("N_max", self.N_max), ("NLLR_upperLimit", self.scoreUpperLimit), ("pruneThreshold", self.pruneThreshold),
                            ("targetSizeLimit", self.targetSizeLimit), ("maxSpeedMS", self.maxSpeedMS)):
            ET.SubElement(settings, name).text = str(value)

    def _storeRun(self, scenarioElement, preInitialized=True, smooth=False, constantTurn=False, ais=False, em=0, emStart="model", **kwargs):
        """One <Run>: the per-stage run times of every scan and one <Track> per live and per terminated target -- all states of
        the selected hypothesis' chain (preInitialized=True) or its first and last.  smooth=True also fills every track's
        <SmoothedStates> (one <S> per node), all tracks of the run smoothed in ONE device call (getSmoothTracks, which constantTurn is
        handed to: a constant-turn tracker smooths with constantTurn=True only; so is ais: an AIS-aided tracker's smoothed states hold
        its AIS updates with ais=True only; and em, emStart, which are then -- for em > 0 only -- also written as attributes of every
        <SmoothedStates>); by default the element stays empty."""
        import xml.etree.ElementTree as ET
        run = ET.SubElement(scenarioElement, xmltags.runTag)
        run.attrib[xmltags.iterationTag] = str(kwargs[xmltags.iterationTag] if xmltags.iterationTag in kwargs
                                               else len(scenarioElement.findall(xmltags.runTag)))
        if xmltags.seedTag in kwargs:
            run.attrib[xmltags.seedTag] = str(kwargs[xmltags.seedTag])
        prec = xmltags.timeLogPrecision
        runtime = ET.SubElement(run, xmltags.runtimeTag, attrib={xmltags.descriptionTag: "Per iteration", xmltags.precisionTag: str(prec)})
        for stage, values in self.runtimeLog.items():
            if not values:
                continue
            v = np.array(values)
            ET.SubElement(runtime, str(stage), attrib={xmltags.meanTag: str(round(np.mean(v), prec)), xmltags.minTag: str(round(np.min(v), prec)),
                                                       xmltags.maxTag: str(round(np.max(v), prec))}
                          ).text = np.array_str(v, precision=prec, max_line_width=999999)
        groups = ((list(self.__trackNodes__), {}), (self.__terminatedTargets__, {xmltags.terminatedTag: True}))
        smoothed = (iter(self._smooth_nodes([node for nodes, _ in groups for node in nodes], constantTurn=constantTurn, ais=ais, em=em, emStart=emStart))
                    if (smooth and preInitialized) else None)
        for nodes, extra in groups:
            for node in nodes:
                if preInitialized:
                    track = node._storeNode(run, self.radarPeriod, smooth=(next(smoothed) if smoothed is not None else False), **extra)
                    if smoothed is not None and em > 0:
                        track.find(xmltags.smoothedstatesTag).attrib.update({"em": str(em), "emStart": emStart})
                else:
                    node._storeNodeSparse(run, **extra)
        return run

    def getRuntimeAverage(self):
        return {k: np.mean(np.array(v)) for k, v in self.runtimeLog.items() if len(v)}

    def _findClustersFromSets(self):
        return self.__clusterList__

    def close(self):
        self._pendq = []
        if self.initiator is not None:
            self.initiator.close()
            self.initiator = None
        self._ctx.close()
