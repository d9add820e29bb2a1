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
        plan_of(A, self.num_nodes, self.layers["layer_0"].num_relations, operand_row_bytes=self.operand_row_bytes())
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
