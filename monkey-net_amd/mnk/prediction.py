"""The prediction task (prediction.py) as a batched engine: `Prediction.extract` (prediction.py:64-74), `Prediction.fit`
(prediction.py:76-111) and `Prediction.predict` (prediction.py:117-133) on the kernels of csrc/predict.hip and csrc/gru.hip.

* extract: the key points of the training videos by detector calls of many frames each (the detector folds frames into the
  batch), kept on the device as one pool of rows -- a row is one frame of the predictor's input (prediction_module.py:28-33).
* fit: one iteration is a fixed list of kernel launches on one stream -- window gather, input projection, T recurrent steps,
  linear layer, the L1 loss fused with the output head, its gradient, the backward kernels, one MnkAdam step -- with every
  buffer allocated once per batch size; the weight gradients are written straight into the optimiser's flat buffer.  No
  autograd tape, no stock-operator launch.  With use_graph the list is captured once per batch size as ONE linear hipGraph and
  replayed with the window starts copied into a static buffer.  The host reads one number per epoch (the mean loss, for
  ReduceLROnPlateau).
* predict: B videos at once -- one detector call, the roll-out, one generator call with the source encoded once.

PyTorch provides memory, streams and the optimiser / scheduler objects only."""
import numpy as np
import torch

from . import _lib
from . import graphs as mgraphs
from . import gru as mgru
from . import ops as mops
from .ops import _p


class KeyPointPool:
    """rows: [total_frames, I] fp32 on the device (all means [K][2], then with 'var' all covariances [K][2][2], per frame);
    videos: [(offset, frame_count)] of every video, in dataset order."""

    def __init__(self, rows, videos):
        assert rows.dim() == 2 and rows.dtype == torch.float32 and rows.is_contiguous()
        self.rows = rows
        self.videos = [(int(o), int(n)) for o, n in videos]
        assert all(o >= 0 and n >= 0 and o + n <= rows.shape[0] for o, n in self.videos)

    def __len__(self):
        return len(self.videos)

    def video(self, i):
        o, n = self.videos[i]
        return self.rows[o:o + n]


def kp_rows(kp):
    """a key-point dict (mean [..., K, 2], var [..., K, 2, 2]) as predictor-input rows [frames, I] (prediction_module.py:28-33)"""
    n = kp["mean"].shape[:-2].numel()
    return torch.cat([kp[k].reshape(n, -1) for k in ("mean", "var") if k in kp], dim=-1)


class _Plan:
    """The buffers and the launch list of one batch size: every argument of every launch is fixed when the plan is built."""

    def __init__(self):
        self.ops = []           # (entry point, argument tuple without the stream)
        self.keep = []          # tensors whose addresses the launch list holds
        self.graph = None

    def add(self, name, *args):
        self.ops.append((name, args))

    def run(self, stream):
        call = _lib.lib().call
        for name, args in self.ops:
            call(name, *args, stream)


class Prediction:
    """prediction.py:55-133 without its per-frame and per-window host work.

    prediction_params: the YAML section -- rnn_params, predict_variance, num_epochs, lr, batch_size, num_frames, init_frames and
    train_size are read.  precision / fuse_norm / skinny: one ops.EvalOptions value, as in Reconstructor; they apply to the
    detector and generator calls only (the GRU runs in fp32).  frames_per_call: the most frames one detector call of extract()
    takes.  patience: ReduceLROnPlateau's (prediction.py:87).  rng: a numpy RandomState / Generator-like object with .choice
    for the window starts; None: the global np.random, so a seeded run draws the reference's windows (augmentation.py:339).
    use_graph: capture the training iteration as a hipGraph; None: on a device build (the emulator always runs eager).

    .predictor is a mnk.predictor.PredictionModule with the reference's state_dict keys and seeded initial weights.  It is created
    where prediction.py:76 creates its own: on first use after extract() -- by fit(), predict() or by reading the attribute.

    The one deliberate difference from the reference: a video shorter than num_frames raises ValueError in extract() (the
    reference takes the shorter window and fails in the DataLoader's collation unless every video is equally short).
    num_frames <= init_frames raises too: the reference's loss would be the mean of an empty slice.  Dropout between stacked GRU
    layers in training mode (dropout > 0 with num_layers > 1; no shipped configuration) is refused."""

    def __init__(self, kp_detector, generator, prediction_params, num_kp, kp_variance, use_graph=None, precision="fp32",
                 fuse_norm=False, skinny=False, frames_per_call=32, patience=50, rng=None):
        self.kp_detector = kp_detector.eval() if kp_detector is not None else None      # (None: an engine for fit() alone)
        self.generator = generator.eval() if generator is not None else None
        self.options = mops.EvalOptions(mops.check_precision(precision), bool(fuse_norm), bool(skinny))
        self.precision, self.fuse_norm, self.skinny = self.options
        self.params = dict(prediction_params)
        self.num_kp, self.kp_variance = int(num_kp), kp_variance
        self.has_var = kp_variance == 'matrix'
        self.feats = 6 if self.has_var else 2
        self.row = self.num_kp * self.feats
        self.num_frames, self.init_frames = int(self.params["num_frames"]), int(self.params["init_frames"])
        if self.num_frames <= self.init_frames:
            raise ValueError("num_frames (%d) must exceed init_frames (%d): the loss of prediction.py:103 would be the mean of an "
                             "empty slice" % (self.num_frames, self.init_frames))
        if self.init_frames < 1:
            raise ValueError("init_frames must be at least 1")
        rnn = dict(self.params.get("rnn_params") or {})
        if rnn.get("num_layers", 1) > 1 and rnn.get("dropout", 0.5) > 0:
            raise ValueError("dropout between stacked GRU layers in training mode is not served by the prediction engine")
        self.use_graph = use_graph
        self.frames_per_call = int(frames_per_call)
        self.patience = int(patience)
        self.rng = rng
        self._predictor = None
        self.optimizer = self.scheduler = None
        self._plans = {}
        self._acc = self._log = self._epoch_starts = None
        self._iters = 0
        self._dev = None                # the pool's device, where there is no detector to take it from

    # ---- the predictor and its optimiser ----------------------------------------------------------------------------------
    @property
    def device(self):
        if self.kp_detector is not None:
            return next(self.kp_detector.parameters()).device
        return self._dev if self._dev is not None else torch.device("cpu")

    @property
    def predictor(self):
        if self._predictor is None:
            from .predictor import PredictionModule
            self._predictor = PredictionModule(num_kp=self.num_kp, kp_variance=self.kp_variance,
                                               **(self.params.get("rnn_params") or {})).to(self.device)
        return self._predictor

    def _graph_on(self):
        on_device = _lib.lib().is_device_build and self.device.type == "cuda"
        return on_device if self.use_graph is None else (bool(self.use_graph) and on_device)

    def _optimizer(self):
        if self.optimizer is None:
            from .optim import MnkAdam
            self.optimizer = MnkAdam(self.predictor.parameters(), lr=self.params["lr"])
            self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, patience=self.patience)
        return self.optimizer

    # ---- extract ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def extract(self, videos):
        """videos: an iterable of (1, C, F, H, W) device tensors, in dataset order (prediction.py:64-74 keeps train_size + 1 of
        them: it breaks on `it > train_size`).  Returns the KeyPointPool; nothing goes to the host."""
        train_size = self.params.get("train_size")
        pending, npending, chunks, index, off = [], 0, [], [], 0

        def detect(n):
            nonlocal pending, npending
            take, rest, need = [], [], n
            for v in pending:
                if need >= v.shape[2]:
                    take.append(v)
                    need -= v.shape[2]
                elif need > 0:
                    take.append(v[:, :, :need])
                    rest.append(v[:, :, need:])
                    need = 0
                else:
                    rest.append(v)
            pending, npending = rest, npending - n
            with mops.eval_options(*self.options):
                kp = self.kp_detector(take[0] if len(take) == 1 else torch.cat(take, dim=2))
            chunks.append(kp_rows(kp))

        for it, v in enumerate(videos):
            if train_size is not None and it > train_size:
                break
            if v.dim() != 5 or v.shape[0] != 1:
                raise ValueError("video %d: expected a (1, C, F, H, W) tensor, got %s" % (it, tuple(v.shape)))
            if v.shape[2] < self.num_frames:
                raise ValueError("video %d has %d frames, fewer than num_frames = %d" % (it, v.shape[2], self.num_frames))
            mops._check_device(v)
            index.append((off, int(v.shape[2])))
            off += int(v.shape[2])
            pending.append(v)
            npending += int(v.shape[2])
            while npending >= self.frames_per_call:
                detect(self.frames_per_call)
        if npending:
            detect(npending)
        if not chunks:
            raise ValueError("no videos")
        rows = chunks[0] if len(chunks) == 1 else torch.cat(chunks, dim=0)
        assert rows.shape == (off, self.row), (rows.shape, off, self.row)
        self.predictor                      # prediction.py:76: created behind the extraction
        return KeyPointPool(rows.contiguous(), index)

    # ---- the launch lists -----------------------------------------------------------------------------------------------------
    def _gemm(self, plan, transA, transB, M, N, K, A, B, C, bias=None):
        ws_n = mops._query("mnk_gru_gemm_workspace_floats", M, N, K)
        ws = torch.empty(ws_n, dtype=torch.float32, device=C.device) if ws_n else None
        lda, ag, ldag = mgru._rows(A)
        ldb, bg, ldbg = mgru._rows(B)
        plan.keep += [A, B, C, bias, ws]
        plan.add("mnk_gru_gemm", transA, transB, M, N, K, _p(A), lda, ag, ldag, _p(B), ldb, bg, ldbg, _p(bias), _p(C), N, _p(ws), ws_n)

    def _colsum(self, plan, x2d, out):
        rows, cols = x2d.shape
        ws_n = mops._query("mnk_gru_colsum_workspace_floats", rows, cols)
        ws = torch.empty(max(ws_n, 1), dtype=torch.float32, device=x2d.device)
        plan.keep += [x2d, out, ws]
        plan.add("mnk_gru_colsum", _p(x2d), x2d.stride(0), rows, cols, _p(out), _p(ws), ws_n)

    def _layers(self):
        rnn = self.predictor.rnn
        return [tuple(getattr(rnn, "%s_l%d" % (n, l)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                for l in range(rnn.num_layers)]

    def _forward_ops(self, plan, x, B, T, train):
        """input projection, T step launches and the linear layer of every GRU layer on x [B, T, I]: (y [B, T, I], per-layer
        (input, gi, hs, gates))"""
        dev, H = x.device, self.predictor.rnn.hidden_size
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        saved, inp = [], x
        for w_ih, w_hh, b_ih, b_hh in self._layers():
            gi, hs = new(T, B, 3 * H), new(T + 1, B, H)
            hs[0].zero_()                                   # h0 = 0: written once, no launch ever writes it again
            gates = new(T, B, 4 * H) if train else None
            self._gemm(plan, 0, 1, T * B, 3 * H, inp.shape[2], inp.transpose(0, 1), w_ih, gi, b_ih)
            for t in range(T):
                plan.add("mnk_gru_step_fwd", _p(hs[t]), H, _p(w_hh), _p(b_hh), _p(gi[t]), 3 * H, _p(hs[t + 1]), H,
                         _p(gates[t]) if train else None, B, H)
            plan.keep += [hs, gi, gates, w_hh, b_hh]
            saved.append((inp, gi, hs, gates))
            inp = hs[1:].transpose(0, 1)                    # [B, T, H] read where it lies (grouped rows)
        lin = self.predictor.linear
        y = new(B, T, self.row)
        self._gemm(plan, 0, 1, B * T, self.row, H, inp, lin.weight, y, lin.bias)
        return y, saved, inp

    def _param_key(self):
        return tuple(p.data_ptr() for p in self.predictor.parameters())

    def _train_plan(self, pool, B):
        key = ("train", B, pool.rows.data_ptr(), pool.rows.shape[0], _p(self._log), self._param_key())
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        plan = self._plans[key] = _Plan()
        opt = self._optimizer()
        dev, T, K, F, I, H = pool.rows.device, self.num_frames, self.num_kp, self.feats, self.row, self.predictor.rnn.hidden_size
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        plan.starts = torch.zeros(B, dtype=torch.int64, device=dev)
        x, gt = new(B, T, I), new(B, T, I)
        plan.x, plan.gt = x, gt
        plan.keep += [pool.rows, x, gt]
        # op 0, the gather: _iteration passes the address of this iteration's starts itself
        plan.gather = (_p(pool.rows), pool.rows.shape[0], pool.rows.stride(0), B, T, self.init_frames, I, _p(x), _p(gt))
        y, saved, top = self._forward_ops(plan, x, B, T, True)
        ws_n = mops._query("mnk_gru_head_l1_workspace_floats", B, T, K)
        plan.loss, ws, dy = new(1), new(ws_n), new(B * T, I)
        plan.keep += [y, ws, dy]
        plan.add("mnk_gru_head_l1_fwd", _p(y), _p(gt), B, T, K, F, int(self.has_var), self.init_frames, _p(plan.loss), _p(self._acc),
                 _p(self._log), self._log.numel(), _p(ws), ws_n)
        plan.add("mnk_gru_head_l1_bwd", _p(y), _p(gt), B, T, K, F, int(self.has_var), self.init_frames, _p(dy))
        lin = self.predictor.linear
        dout = new(B, T, H)
        self._gemm(plan, 0, 0, B * T, H, I, dy, lin.weight, dout)
        self._gemm(plan, 1, 0, I, H, B * T, dy, top, opt.sink(lin.weight))
        self._colsum(plan, dy, opt.sink(lin.bias))
        for l in range(len(saved) - 1, -1, -1):
            inp, gi, hs, gates = saved[l]
            w_ih, w_hh, b_ih, b_hh = self._layers()[l]
            dgi, dgh, carry = new(T, B, 3 * H), new(T, B, 3 * H), new(B, H)
            plan.keep += [dout, dgi, dgh, carry]
            ld_dy = dout.stride(0)
            plan.add("mnk_gru_gates_bwd", _p(dout[:, T - 1]), ld_dy, None, _p(gates[T - 1]), _p(hs[T - 1]), H, _p(dgi[T - 1]),
                     _p(dgh[T - 1]), _p(carry), B, H)
            for t in range(T - 1, 0, -1):
                plan.add("mnk_gru_step_bwd", _p(dgh[t]), _p(w_hh), _p(carry), _p(dout[:, t - 1]), ld_dy, _p(gates[t - 1]),
                         _p(hs[t - 1]), H, _p(dgi[t - 1]), _p(dgh[t - 1]), None, H, B, H)
            Il = inp.shape[2]
            if l > 0:
                dxt = new(T, B, Il)
                self._gemm(plan, 0, 0, T * B, Il, 3 * H, dgi, w_ih, dxt)
                dout = dxt.transpose(0, 1)
            self._gemm(plan, 1, 0, 3 * H, Il, T * B, dgi, inp.transpose(0, 1), opt.sink(w_ih))
            self._gemm(plan, 1, 0, 3 * H, H, T * B, dgh, hs[:T], opt.sink(w_hh))
            self._colsum(plan, dgi.view(T * B, 3 * H), opt.sink(b_ih))
            self._colsum(plan, dgh.view(T * B, 3 * H), opt.sink(b_hh))
        return plan

    def _iteration(self, plan, starts):
        """one iteration of prediction.py:96-107 on the windows whose first pool rows `starts` (device, int64) holds"""
        stream = mops._stream(plan.x)
        g = plan.gather
        _lib.lib().call("mnk_kp_window_gather", g[0], g[1], g[2], _p(starts), *g[3:], stream)
        plan.run(stream)
        opt = self.optimizer
        opt._written.update(id(p) for p in opt._params)    # every sink was written by the launches above
        opt.step()

    def _snapshot(self):
        opt = self.optimizer
        return ([p.detach().clone() for p in opt._params], opt.flat_m.clone(), opt.flat_v.clone(), opt.hyper.clone(),
                self._acc.clone(), self._log.clone(), opt.steps_taken)

    def _restore(self, snap):
        opt = self.optimizer
        with torch.no_grad():
            for p, c in zip(opt._params, snap[0]):
                p.copy_(c)
            opt.flat_m.copy_(snap[1])
            opt.flat_v.copy_(snap[2])
            # what a step advances: the bias corrections [4:6] and the step counter [7] (the learning rate stays as synced)
            opt.hyper[4:6].copy_(snap[3][4:6])
            opt.hyper[7:8].copy_(snap[3][7:8])
            self._acc.copy_(snap[4])
            self._log.copy_(snap[5])
        opt.steps_taken = snap[6]

    def _capture(self, plan):
        """the iteration as ONE hipGraph on one stream: a warm-up iteration (it builds the optimiser's descriptor table), the
        capture, then parameters, optimiser state and accumulators put back, so that every replay applies exactly one update"""
        snap = self._snapshot()
        mgraphs.warm_up(lambda: self._iteration(plan, plan.starts), 1)
        plan.graph, _ = mgraphs.capture(lambda: self._iteration(plan, plan.starts))
        self._restore(snap)

    # ---- fit ----------------------------------------------------------------------------------------------------------------
    def draw_starts(self, pool):
        """one window start per video, in dataset order, as augmentation.py:339 draws it; as pool rows"""
        rng = np.random if self.rng is None else self.rng
        return [o + int(rng.choice(max(1, n - self.num_frames + 1), size=1)[0]) for o, n in pool.videos]

    def fit(self, pool, num_epochs=None, on_epoch=None):
        """prediction.py:94-111.  Returns the epoch mean losses; on_epoch(epoch, mean_loss) is called after every epoch
        (iteration_losses() then holds that epoch's losses).  Per epoch one window start per video is drawn in dataset order
        (draw_starts); the draws of epoch e + 1 are made while the device works on epoch e -- the generator sees the same
        sequence of calls as in the reference, and nothing is drawn beyond the last epoch.  The epoch mean is the device's
        sequential fp32 sum of the iteration losses divided on the host."""
        if any(n < self.num_frames for _, n in pool.videos):
            raise ValueError("a video of the pool has fewer than num_frames = %d frames" % self.num_frames)
        mops._check_device(pool.rows)
        self._dev = pool.rows.device
        if self.optimizer is None:
            self.predictor.to(self._dev)        # (an engine without a detector makes its predictor on the CPU)
        num_epochs = self.params["num_epochs"] if num_epochs is None else num_epochs
        bs, n = int(self.params["batch_size"]), len(pool)
        opt = self._optimizer()
        self.predictor.train()
        dev = pool.rows.device
        iters = (n + bs - 1) // bs
        if self._acc is None or self._log.numel() != iters or self._acc.device != dev:
            self._acc = torch.zeros(2, dtype=torch.float32, device=dev)
            self._log = torch.zeros(iters, dtype=torch.float32, device=dev)
            self._epoch_starts = torch.zeros(n, dtype=torch.int64, device=dev)
        graph = self._graph_on()
        history = []
        starts = self.draw_starts(pool) if num_epochs > 0 else None
        for epoch in range(num_epochs):
            self._epoch_starts.copy_(torch.tensor(starts, dtype=torch.int64))
            self._acc.zero_()
            for i in range(0, n, bs):
                b = min(bs, n - i)
                plan = self._train_plan(pool, b)
                if not graph:
                    self._iteration(plan, self._epoch_starts[i:i + b])
                    continue
                if plan.graph is None:
                    self._capture(plan)
                opt.sync_scalars()                          # a lowered learning rate reaches the device scalars of the replay
                plan.starts.copy_(self._epoch_starts[i:i + b], non_blocking=True)
                plan.graph.replay()
                opt.steps_taken += 1
            self._iters = iters
            # the next epoch's windows, drawn while the device works on this one: the draws are host work (a numpy call per
            # video, microseconds each -- per iteration as long as the launches) and the generator sees them in the same order
            if epoch + 1 < num_epochs:
                starts = self.draw_starts(pool)
            loss = float(self._acc[0:1].cpu()[0]) / iters   # the one number the host reads per epoch (np.mean(loss_list))
            self.scheduler.step(loss)
            history.append(loss)
            if on_epoch is not None:
                on_epoch(epoch, loss)
        return history

    def iteration_losses(self):
        """the losses of the last epoch's iterations (a device tensor; a copy)"""
        return self._log[:self._iters].clone()

    # ---- predict --------------------------------------------------------------------------------------------------------------
    def _eval_plan(self, B, dev):
        key = ("eval", B, str(dev), self._param_key())
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        plan = self._plans[key] = _Plan()
        T, K, F, I = self.num_frames, self.num_kp, self.feats, self.row
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        plan.starts = torch.arange(B, dtype=torch.int64, device=dev) * T
        plan.x, plan.gt = new(B, T, I), new(B, T, I)
        plan.y, _, _ = self._forward_ops(plan, plan.x, B, T, False)
        return plan

    @torch.no_grad()
    def predict(self, video):
        """prediction.py:119-133 for B videos at once: video (B, C, >= num_frames, H, W) -> the dict reconstruction.generate
        returns (video_prediction, video_deformed: (B, C, num_frames, H, W); kp_driving: the rolled-out key points; kp_source:
        the key points of frame 0) plus kp_init, the masked key points the roll-out started from.
        predict_variance keeps the reference's meaning: SET means the covariances are NOT predicted -- every frame gets the
        covariance of frame init_frames - 1 (prediction.py:129-131); unset, the GRU's own covariances are used."""
        if video.dim() != 5 or video.shape[2] < self.num_frames:
            raise ValueError("expected (B, C, >= %d, H, W), got %s" % (self.num_frames, tuple(video.shape)))
        mops._check_device(video)
        B, T, K, F, I = video.shape[0], self.num_frames, self.num_kp, self.feats, self.row
        if self.optimizer is None:
            self.predictor.to(video.device)
        self.predictor.eval()
        clip = video[:, :, :T]
        with mops.eval_options(*self.options):
            kp = self.kp_detector(clip)
        kp_source = {k: v[:, :1] for k, v in kp.items()}
        rows = kp_rows(kp)
        plan = self._eval_plan(B, video.device)
        stream = mops._stream(rows)
        call = _lib.lib().call
        call("mnk_kp_window_gather", _p(rows), rows.shape[0], rows.stride(0), _p(plan.starts), B, T, self.init_frames, I, _p(plan.x),
             _p(plan.gt), stream)
        plan.run(stream)
        mean = torch.empty(B, T, K, 2, dtype=torch.float32, device=video.device)
        var = torch.empty(B, T, K, 2, 2, dtype=torch.float32, device=video.device) if self.has_var else None
        call("mnk_gru_head_fwd", _p(plan.y), B * T, K, F, int(self.has_var), _p(mean), _p(var), stream)
        call("mnk_kp_rollout_finish", _p(plan.x), I, B, T, K, int(self.has_var), self.init_frames,
             int(bool(self.params.get("predict_variance"))), _p(mean), _p(var), stream)
        kp_video = {"mean": mean, "var": var} if self.has_var else {"mean": mean}
        x = plan.x.clone()
        kp_init = {"mean": x[..., :2 * K].view(B, T, K, 2)}
        if self.has_var:
            kp_init["var"] = x[..., 2 * K:].view(B, T, K, 2, 2)
        with mops.eval_options(*self.options):
            out = self.generator(clip[:, :, :1], kp_driving=kp_video, kp_source=kp_source)
        return {"video_prediction": out["video_prediction"], "video_deformed": out["video_deformed"], "kp_driving": kp_video,
                "kp_source": kp_source, "kp_init": kp_init}
