"""Stack of R-GCN layers behind the reference's `RGCN` interface (mrgcn/models/rgcn.py:12-132):
same constructor, `layers` / `activations` ModuleDicts keyed `layer_<i>`, `relations` table for
link prediction, `num_layers`.  In full-batch mode the ReLU between layers is folded into the
epilogue of the layer's sparse product; mini-batch mode (`A_Batch` input) walks the row slices."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.nn.functional import dropout

from ..layers.graph import GraphConvolution
from ..plan import build_plans_parallel, plan_of


class _DrawState:
    """{seed, position} of a device draw with node dropout's semantics: host words until the first forward makes the
    int64 pair in device memory, then that pair — written in place, so a captured step keeps reading the same words."""

    def __init__(self, what: str):
        self.what, self.seed, self.position, self.state = what, None, 0, None

    def device_state(self, device):
        from .. import _lib
        from .. import functional as Fn
        st = self.state
        if st is None or st.device != device:
            if st is not None:
                self.seed, self.position = self.word(0), self.word(1)
            if torch.cuda.is_current_stream_capturing():
                raise _lib.MrgcnError(f"{self.what}: the device state is made by the first forward; run one step "
                                      "before capturing")
            if self.seed is None:
                self.seed = torch.initial_seed()
            st = self.state = Fn.node_dropout_state(self.seed, self.position, device)
        return st

    def word(self, i):
        if self.state is None:
            v = (self.seed, self.position)[i]
            return (torch.initial_seed() if v is None else int(v)) & 0xFFFFFFFFFFFFFFFF
        return int(self.state[i].item()) & 0xFFFFFFFFFFFFFFFF   # (a read-back: not for the inside of a step)

    def set_word(self, i, value):
        from .. import functional as Fn
        value = int(value) & 0xFFFFFFFFFFFFFFFF
        other = self.word(1 - i)
        if i == 0:
            self.seed = value
        else:
            self.position = value
        if self.state is not None:   # in place: a captured step keeps reading the same words
            pair = (value, other) if i == 0 else (other, value)
            self.state.copy_(Fn.node_dropout_state(pair[0], pair[1], self.state.device))


def refuse_edge_dropout(model, what: str):
    """Raises when `model` (or a module inside it) would draw edge dropout in its next forward: for the steps whose
    backward cannot run on a value overlay."""
    from .. import _lib
    for m in model.modules():
        if isinstance(m, RGCN) and m._edge_dropout_active():
            raise _lib.MrgcnError(f"edge dropout: {what} is outside what runs on a value overlay of the plan (full-batch "
                                  "forward, dense output gradient: tasks.link_prediction.train_step / fit / GraphedStep, "
                                  "or a plain loss.backward()); set_edge_dropout(0.0) for this step")


class RGCN(nn.Module):
    def __init__(self, modules, num_relations, num_nodes, num_bases, p_dropout, featureless, bias,
                 link_prediction, num_blocks=-1):
        super().__init__()
        assert len(modules) > 0

        self.num_nodes = num_nodes
        self.p_dropout = p_dropout
        self.layers = nn.ModuleDict()
        self.activations = nn.ModuleDict()
        for i, (indim, outdim, _ltype, f_activation) in enumerate(modules):
            first = i == 0  # rgcn.py:30-37: only layer 0 is an input layer / may be featureless
            # block-diagonal weights (num_blocks > 0) go to every layer that has a feature term; a featureless
            # layer 0 keeps its bases
            has_F = not (first and featureless)
            self.layers[f"layer_{i}"] = GraphConvolution(
                indim=indim, outdim=outdim, num_relations=num_relations, num_nodes=num_nodes,
                num_bases=num_bases, featureless=featureless if first else False,
                input_layer=first, bias=bias, num_blocks=num_blocks if has_F else -1)
            self.activations[f"layer_{i}"] = f_activation
        self.num_layers = len(self.layers)
        # hidden layers keep their output in rows padded to whole 16-byte pieces (plan.spmm: the product stores whole
        # pieces); the model's own output is dense like the reference's
        for key in list(self.layers)[:-1]:
            self.layers[key].padded_output = True

        # node dropout (p_dropout > 0): "host" draws on the CPU as the reference does, "device" on the GPU inside the
        # layers' own functions (set_node_dropout).  None of this is a parameter or a buffer: state_dict keys are API.
        self.node_dropout_mode = "host"
        self.node_dropout_masks = None   # an explicit list of per-layer device masks, used instead of drawing
        self.last_node_masks = []        # the masks of the last device-mode forward (references, not copies)
        self._node_dropout_seed, self._node_dropout_position = None, 0   # until the device state exists
        self._node_dropout_state = None  # int64 {seed, position} in device memory

        # edge dropout (set_edge_dropout): per-relation rates, a device state of its own, one value overlay of the
        # adjacency's plan per layer.  None of this is a parameter or a buffer either.
        self._edge_rates = None          # R host floats, or None: off
        self._edge_rescale = True
        self._edge_state = _DrawState("edge dropout")
        self._edge_rates_dev = {}        # device -> fp32 [R]
        self._edge_plans = {}            # id(plan) -> (plan, [overlay per layer])
        self.last_edge_plans = []        # the overlays of the last training forward (references)

        if link_prediction:
            # DistMult diagonal relation embeddings (rgcn.py:55-61)
            self.relations = nn.Parameter(torch.empty((num_relations, modules[-1][1])))
            self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.relations)

    def set_engine(self, engine: str):
        for layer in self.layers.values():
            layer.engine = engine

    def set_operand_dtype(self, dtype: str):
        assert dtype in ("f32", "bf16")
        for layer in self.layers.values():
            layer.operand_dtype = dtype

    # -- node dropout ----------------------------------------------------------------------------------------------
    def set_node_dropout(self, mode: str, seed=None):
        """Where the node masks of `p_dropout > 0` come from.  "host" (the default): the reference's own sequence, a
        CPU draw from torch's generator per layer, copied over and multiplied in (rgcn.py:78-84) — also in `eval()`,
        as there.  "device": drawn on the GPU with Philox4x32-10 from (seed, stream position, layer, node) and applied
        inside the layers' fused functions; the position lives in device memory and moves on after every forward, so
        the step holds no host draw, no copy and no synchronisation and can be captured and replayed
        (`train.GraphedTrainStep`, `GraphedStep`).  Fused engine only.  `seed`: None keeps the current one (at first
        torch's initial seed)."""
        if mode not in ("host", "device"):
            raise ValueError(f"node dropout mode {mode!r}: 'host' or 'device'")
        if mode == "device":
            self._check_device_dropout_engine()
        self.node_dropout_mode = mode
        if seed is not None:
            self.node_dropout_seed = seed
        return self

    def _check_device_dropout_engine(self):
        from .. import _lib
        bad = [k for k, layer in self.layers.items() if layer.engine != "fused"]
        if bad:
            raise _lib.MrgcnError(f"node dropout on the device runs on the fused engine; {', '.join(bad)} use the "
                                  f"'{self.layers[bad[0]].engine}' engine (set_node_dropout('host'), or set_engine('fused'))")

    def _dropout_state(self, device):
        from .. import functional as Fn
        st = self._node_dropout_state
        if st is None or st.device != device:
            if st is not None:
                self._node_dropout_seed, self._node_dropout_position = self.node_dropout_seed, self.node_dropout_position
            if torch.cuda.is_current_stream_capturing():
                from .. import _lib
                raise _lib.MrgcnError("node dropout: the device state is made by the first forward; run one step "
                                      "before capturing")
            if self._node_dropout_seed is None:
                self._node_dropout_seed = torch.initial_seed()
            st = self._node_dropout_state = Fn.node_dropout_state(self._node_dropout_seed, self._node_dropout_position,
                                                                  device)
        return st

    def _state_word(self, i):
        st = self._node_dropout_state
        if st is None:
            v = (self._node_dropout_seed, self._node_dropout_position)[i]
            return (torch.initial_seed() if v is None else int(v)) & 0xFFFFFFFFFFFFFFFF
        return int(st[i].item()) & 0xFFFFFFFFFFFFFFFF   # (a read-back: not for the inside of a step)

    def _set_state_word(self, i, value):
        from .. import functional as Fn
        value = int(value) & 0xFFFFFFFFFFFFFFFF
        if i == 0:
            self._node_dropout_seed = value
        else:
            self._node_dropout_position = value
        st = self._node_dropout_state
        if st is not None:   # in place: a captured step keeps reading the same words
            other = self._state_word(1 - i)
            pair = (value, other) if i == 0 else (other, value)
            st.copy_(Fn.node_dropout_state(pair[0], pair[1], st.device))

    node_dropout_seed = property(lambda self: self._state_word(0), lambda self, v: self._set_state_word(0, v),
                                 doc="seed of the device draw (64 bits)")
    node_dropout_position = property(lambda self: self._state_word(1), lambda self, v: self._set_state_word(1, v),
                                     doc="stream position of the device draw: the number of device-mode forwards so "
                                         "far (each one takes the masks of one position)")

    # -- edge dropout ----------------------------------------------------------------------------------------------
    def set_edge_dropout(self, p: float = 0.0, self_loop=None, rates=None, rescale: bool = True, seed=None):
        """Edge dropout on the device (Schlichtkrull et al. 2018, §5: 0.4 on ordinary edges, 0.2 on self-loops): in
        `train()` mode every full-batch forward draws, per graph-convolution layer, which entries of the adjacency are
        dropped — Philox4x32-10 keyed by (seed, position, layer, row, source node, relation), csrc/edge_dropout.hip —
        into a value overlay of the plan (`GraphPlan.overlay()`), and the layer computes on that overlay, forward and
        backward.  `p`: the rate of every relation but the last; `self_loop`: the rate of the last relation, the
        identity block (None: `p`); `rates`: one rate per relation instead of both.  Each rate in [0, 1).  `rescale`:
        kept entries are multiplied by 1 / (1 - rate).  `eval()` forwards use the plan itself and draw nothing.  With
        every rate zero the model runs exactly as without the call.  Fused engine, full-batch plans only.  `seed`: None
        keeps the current one (at first torch's initial seed)."""
        R = int(self.layers["layer_0"].num_relations)
        if rates is None:
            rates = [float(p)] * (R - 1) + [float(p if self_loop is None else self_loop)]
        else:
            rates = [float(r) for r in rates]
            if len(rates) != R:
                raise ValueError(f"edge dropout: {len(rates)} rates for {R} relations")
        for r in rates:
            if not 0.0 <= r < 1.0:
                raise ValueError(f"edge dropout rates lie in [0, 1), but got {r}")
        if any(r > 0.0 for r in rates):
            self._check_edge_dropout_engine()
            self._edge_rates = rates
        else:
            self._edge_rates = None
        self._edge_rescale = bool(rescale)
        for t in self._edge_rates_dev.values():   # in place: a captured step keeps reading the same vector
            t.copy_(torch.tensor(rates, dtype=torch.float32))
        if seed is not None:
            self.edge_dropout_seed = seed
        return self

    def _check_edge_dropout_engine(self):
        from .. import _lib
        bad = [k for k, layer in self.layers.items() if layer.engine != "fused"]
        if bad:
            raise _lib.MrgcnError(f"edge dropout runs on the fused engine; {', '.join(bad)} use the "
                                  f"'{self.layers[bad[0]].engine}' engine (set_engine('fused'), or set_edge_dropout(0.0))")

    def _edge_dropout_active(self) -> bool:
        return self.training and self._edge_rates is not None

    edge_dropout_seed = property(lambda self: self._edge_state.word(0), lambda self, v: self._edge_state.set_word(0, v),
                                 doc="seed of the edge-dropout draw (64 bits); a state of its own, in no state_dict")
    edge_dropout_position = property(lambda self: self._edge_state.word(1),
                                     lambda self, v: self._edge_state.set_word(1, v),
                                     doc="stream position of the edge-dropout draw: the number of training forwards "
                                         "with edge dropout so far")

    def __getstate__(self):
        # (copies and pickles of the model take no plan handles along: the overlays are made again on first use)
        state = dict(self.__dict__)
        state["_edge_plans"], state["last_edge_plans"], state["_edge_rates_dev"] = {}, [], {}
        return state

    def _edge_overlays(self, plan):
        """The overlays of `plan`, one per layer, drawn for this forward (all of them before the first layer runs: the
        backward of layer l then reads the values its forward read)."""
        from .. import _lib
        self._check_edge_dropout_engine()
        if getattr(plan, "is_overlay", False) or plan.lean:
            raise _lib.MrgcnError("edge dropout draws into overlays of a full-batch plan")
        ent = self._edge_plans.get(id(plan))
        if ent is None or ent[0] is not plan or any(o._h is None for o in ent[1]):
            if torch.cuda.is_current_stream_capturing():
                raise _lib.MrgcnError("edge dropout: the overlays of a plan are made by the first training forward; run "
                                      "one step before capturing")
            while len(self._edge_plans) >= 4:   # (a handful of graphs per model)
                for o in self._edge_plans.pop(next(iter(self._edge_plans)))[1]:
                    o.close()
            ent = self._edge_plans[id(plan)] = (plan, [plan.overlay() for _ in range(self.num_layers)])
        overlays = ent[1]
        dev = plan.device
        st = self._edge_state.device_state(dev)
        rates = self._edge_rates_dev.get(dev)
        if rates is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.MrgcnError("edge dropout: the rate vector is made by the first training forward; run one "
                                      "step before capturing")
            rates = self._edge_rates_dev[dev] = torch.tensor(self._edge_rates, dtype=torch.float32).to(dev)
        for l, o in enumerate(overlays):
            o.draw(rates, st, l, rescale=self._edge_rescale, advance=l == len(overlays) - 1)
        self.last_edge_plans = overlays
        return overlays

    def _device_masks(self, rows, device):
        """The node masks of one forward in device mode, `rows[l]` values for layer l: the explicit
        `node_dropout_masks` when set, else one draw per distinct run of equal sizes, the last one moving the position."""
        from .. import _lib
        from .. import functional as Fn
        self._check_device_dropout_engine()
        if torch.device(device).type != "cuda":
            raise _lib.MrgcnError(f"node dropout on the device needs the batch on a GPU (it is on '{device}'): move the "
                                  "batch over, or set_node_dropout('host')")
        if self.node_dropout_masks is not None:
            masks = list(self.node_dropout_masks)
            if len(masks) != len(rows):
                raise _lib.MrgcnError(f"node_dropout_masks: {len(masks)} masks for {len(rows)} layers")
        else:
            st = self._dropout_state(device)
            masks, l = [], 0
            while l < len(rows):
                k = l + 1
                while k < len(rows) and rows[k] == rows[l]:
                    k += 1
                masks += Fn.node_dropout_draw(st, rows[l], float(self.p_dropout), layers=k - l, layer0=l,
                                              advance=k == len(rows))
                l = k
        self.last_node_masks = masks
        return masks

    def _device_dropout(self) -> bool:
        return self.p_dropout > 0.0 and self.node_dropout_mode == "device"

    def forward(self, X, A):
        if not isinstance(A, torch.Tensor):  # A_Batch (rgcn.py:63-67)
            return self._forward_mini_batch(X, A)
        return self._forward_full_batch(X, A)

    def _forward_mini_batch(self, X, A):
        """rgcn.py:91-128: layer l computes the embeddings of the nodes (L-1-l) hops from the batch
        nodes out of those one hop further, on the matching row slice of A."""
        from ..data.batch import A_BatchMasked, getAdjacencyNodeColumnIdx
        if self._edge_dropout_active():
            from .. import _lib
            raise _lib.MrgcnError("edge dropout: masked and slice mini-batches are outside what runs on a value overlay "
                                  "(a masked batch's supports copy the plan's values; a value refresh for them is "
                                  "future work): full-batch forwards only, or set_edge_dropout(0.0)")
        if isinstance(A, A_BatchMasked):
            return self._forward_masked(X, A)
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            from .. import _lib
            raise _lib.MrgcnError("the mini-batch forward cannot be captured into a hipGraph (its backward decides by "
                                  "counts read back from the device); GraphedTrainStep is for full-batch steps")
        self.prepare_batch(A)
        masks = None
        if self._device_dropout():
            from .. import functional as Fn
            rows = [int(A.row[self.num_layers - (l + 1)].shape[0]) for l in range(self.num_layers)]
            masks = self._device_masks(rows, A.row[0].device)
        for layer_idx, (key, layer) in enumerate(self.layers.items()):
            f_activation = self.activations[key] if key in self.activations else None
            i = self.num_layers - (layer_idx + 1)
            A_slices = A.row[i]
            if layer.input_layer and layer.featureless:
                X = layer(None, A_slices)
            else:
                A_idx = A._a_idx.get(i) if hasattr(A, "_a_idx") else None
                if A_idx is None:
                    A_idx = getAdjacencyNodeColumnIdx(A.neighbours[i], layer.num_nodes,
                                                      layer.num_relations).to(A_slices.device)
                    if hasattr(A, "_a_idx"):
                        A._a_idx[i] = A_idx
                X = layer(X, A_slices, A_idx)
            if masks is not None:
                X = Fn.row_scale(X, masks[layer_idx])   # (the slice layer sums two products: a node of its own)
            elif self.p_dropout > 0.0:
                ones = dropout(torch.ones(X.shape[0]), p=self.p_dropout).to(X.device)
                X = X * ones.unsqueeze(1)
            if f_activation is not None:
                X = f_activation(X)
        return X

    def _forward_masked(self, X, A):
        """The same walk on a masked batch (data.batch.A_BatchMasked): every layer is a masked pass over the full
        graph's plan (functional.masked_layer) on compact arrays — X: one row per node of A.neighbours[-1], hidden
        activations one row per node of the sample they belong to, the result one row per batch node."""
        from .. import _lib
        from .. import functional as Fn
        masks = None
        if self._device_dropout():
            sups = [A.row[self.num_layers - (l + 1)] for l in range(self.num_layers)]
            masks = self._device_masks([int(sup.NR) for sup in sups], sups[0].device)
        for layer_idx, (key, layer) in enumerate(self.layers.items()):
            f_activation = self.activations[key] if key in self.activations else None
            sup = A.row[self.num_layers - (layer_idx + 1)]
            K = 0 if (layer.input_layer and layer.featureless) else int(X.shape[1])
            need_dX = K > 0 and bool(X.requires_grad) and torch.is_grad_enabled()
            if layer.engine != "fused" or not Fn.masked_layer_supported(sup, layer, K, need_dX):
                raise _lib.MrgcnError(
                    f"{key}: outside the masked mini-batch pass (fused engine, f32 operand; out <= 16 with the "
                    "matrix-core transform shapes: an input that wants its gradient has at most 64 columns; or a "
                    "featureless input layer with 1 to 4 bases and 16 < out <= 256, out % 4 == 0; a layer of "
                    "that shape with a feature term on a batch built with wide_features=True, as "
                    "tasks.link_prediction.mkbatches(plan=...) builds them); use data.batch.A_BatchDevice / "
                    "MiniBatch for it")
            fuse_relu = isinstance(f_activation, nn.ReLU) and (self.p_dropout <= 0.0 or masks is not None)
            X = Fn.masked_layer(sup, layer, None if K == 0 else X, relu=fuse_relu,
                                row_scale=masks[layer_idx] if masks is not None else None)
            if masks is None and self.p_dropout > 0.0:
                ones = dropout(torch.ones(X.shape[0]), p=self.p_dropout).to(X.device)
                X = X * ones.unsqueeze(1)
            if f_activation is not None and not fuse_relu:
                X = f_activation(X)
        return X.index_select(0, A.out_rank)

    def prepare_batch(self, A):
        """Builds the slice plans a (fresh) batch still lacks — two per layer at most — side by side.  Called by the
        forward; a prefetcher calls it ahead of time on its own stream (data/batch.py BatchPrefetcher)."""
        jobs = []
        for layer_idx, layer in enumerate(self.layers.values()):
            A_sl = A.row[self.num_layers - (layer_idx + 1)]
            if not (isinstance(A_sl, torch.Tensor) and A_sl.is_cuda):
                continue
            rb = [layer.operand_row_bytes()]
            if layer.input_layer:
                jobs.append((A_sl, layer.num_nodes, layer.num_relations, rb))
            sl = getattr(A_sl, "_mrgcn_slice", None)
            if sl is not None and not (layer.input_layer and layer.featureless):
                jobs.append((sl[1], int(A.neighbours[self.num_layers - (layer_idx + 1)].numel()), layer.num_relations, rb))
        if len(jobs) > 1:
            build_plans_parallel(jobs)
        return A

    def operand_row_bytes(self):
        """Row sizes of the layers' compact operands: the layout hint of the adjacency's graph plan."""
        return sorted({layer.operand_row_bytes() for layer in self.layers.values()})

    def _forward_full_batch(self, X, A):
        # the plan all layers share is built (on first use) for every layer's operand layout
        plan = plan_of(A, self.num_nodes, self.layers["layer_0"].num_relations,
                       operand_row_bytes=self.operand_row_bytes())
        if self._edge_dropout_active():
            # edge dropout: layer l computes on overlay l of the plan, whose values this forward has just drawn
            overlays = self._edge_overlays(plan)
            masks = None
            if self._device_dropout():
                masks = self._device_masks([self.num_nodes] * self.num_layers, X.device if X is not None else A.device)
            for l, (key, layer) in enumerate(self.layers.items()):
                f_activation = self.activations[key] if key in self.activations else None
                fuse_relu = isinstance(f_activation, nn.ReLU) and (masks is not None or self.p_dropout <= 0.0)
                X = layer._forward_fused(X, overlays[l], relu=fuse_relu,
                                         row_scale=masks[l] if masks is not None else None)
                if masks is None and self.p_dropout > 0.0:   # (the host draw, as below)
                    ones = dropout(torch.ones(self.num_nodes), p=self.p_dropout).to(X.device)
                    X = X * ones.unsqueeze(1)
                if f_activation is not None and not fuse_relu:
                    X = f_activation(X)
            return X
        if self._device_dropout():
            # node dropout on the device: the masks of all layers in one draw, each applied inside its layer's function
            # (the ReLU stays in the product's epilogue: relu(m z) = m relu(z) for m >= 0)
            masks = self._device_masks([self.num_nodes] * self.num_layers, X.device if X is not None else A.device)
            for (key, layer), m in zip(self.layers.items(), masks):
                f_activation = self.activations[key] if key in self.activations else None
                fuse_relu = isinstance(f_activation, nn.ReLU)
                X = layer._forward_fused(X, plan_of(A, layer.num_nodes, layer.num_relations), relu=fuse_relu,
                                         row_scale=m)
                if f_activation is not None and not fuse_relu:
                    X = f_activation(X)
            return X
        for key, layer in self.layers.items():
            f_activation = self.activations[key] if key in self.activations else None
            fuse_relu = (isinstance(f_activation, nn.ReLU) and self.p_dropout <= 0.0
                         and layer.engine == "fused")
            if fuse_relu:
                plan = plan_of(A, layer.num_nodes, layer.num_relations)
                X = layer._forward_fused(X, plan, relu=True)
                continue
            X = layer(X, A)
            if self.p_dropout > 0.0:
                # node dropout: one Bernoulli draw per node, applied regardless of train/eval
                # mode and drawn on the CPU, as rgcn.py:78-84 does
                ones = dropout(torch.ones(self.num_nodes), p=self.p_dropout).to(X.device)
                X = X * ones.unsqueeze(1)
            if f_activation is not None:
                X = f_activation(X)
        return X
