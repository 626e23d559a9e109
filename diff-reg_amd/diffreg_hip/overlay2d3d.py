"""Drop-in acceleration of the 2D-3D reverse sampling for an UNMODIFIED Diff-Reg-2d3d checkout.

The loop of MATR2D3D.forward (EXP/model.py:637-694) is inline code: per step it calls, in this order,

    self.get_warped_from_noising_matching3D3D(s_pcd, t_pcd_da, src_mask, tgt_mask_da, x)   -> warped points (+ R, t)      :655-656
    self.denoising_transformer(img_feats, img_dino, img_pixels, pcd_feats, warped)         -> fused img / pcd features   :658-664
    self.denoising_coarse_matching(pcd_feats, img_feats, src_mask, tgt_mask, True)         -> x_start (+ 3 unused)       :665-666

and then updates x with a few element-wise torch ops (:668-680).  `accelerate(model)` re-binds these three call sites ON THE
INSTANCE (the module's weights, state_dict and training branch are untouched): during the first step of an eval forward the
three calls record their arguments, the third one runs the WHOLE loop once in libdiffreg_hip (dr_denoise_loop_2d3d, through
DenoiseEngine2D3D, started from the very x the reference drew) and every step's matching call then hands back the x_start of
that step from the device trace.  The reference's own DDIM arithmetic, final Sinkhorn and read-out (:682-694) run unchanged on
those x_start, so `conf_matrix_pred` and everything behind it are the reference's code on the accelerated loop's values.

    from diffreg_hip.overlay2d3d import accelerate
    model = create_model(cfg).cuda().eval();  accelerate(model)          # EXP/eval.py, after loading the checkpoint

Under model.train() the three calls fall through to the original code -- unless the overlay is installed with `training=True`: then the
four modules of the differentiable training branch (EXP/model.py:386-392, 548, 615-623) -- `transformer`, `denoising_transformer`,
`coarse_matching`, `denoising_coarse_matching` -- run on the device under model.train() (diffreg_hip/autograd2d3d.py: forward and backward in
libdiffreg_hip, gradients into the modules' own parameters and back to the backbone features), and eval forwards keep the loop overlay:

    accelerate(model, training=True);  accelerate_loss(loss_fn)          # EXP/trainval.py, after create_model / OverallLoss(cfg)

accelerate_loss re-binds CoarseMatchingLoss.forward (EXP/loss.py:30-75; an OverallLoss instance: its c_loss) to the device circle + focal loss;
with `fine=True` also FineMatchingLoss.forward (EXP/loss.py:157-215; its f_loss) to the device fine loss (dr_fine_loss_*; the sub-sampling stays
the reference's random_choice).  The GT search, q_sample, the warp and the backbones stay the reference's code -- unless the overlay is
installed with `partition=True`: then the patch partition and the ground-truth patch overlaps between the backbones and the coarse matching
(EXP/model.py:395-540: point_to_node_partition, patchify, get_2d3d_node_correspondences) run on the device (diffreg_hip/partition2d3d.py), and
with `training=True` also the GT search of the training branch (model.py:569: get_correspondences; to_o3d_pcd becomes the identity).  These are
module-level names that forward() calls inline, so they are re-bound in the globals of the module that defines the model's class; `remove()`
restores them.  Without the flag no global is touched.

    accelerate(model, partition=True)                                   # eval
    accelerate(model, training=True, partition=True)                    # training

With `backbone=True` the point backbone in front of all of it (`self.pcd_backbone(pcd_feats, data_dict)`, EXP/model.py:366-368) runs on the device
too, in eval and in train mode (diffreg_hip/pcd_backbone2d3d.py: forward and backward in libdiffreg_hip, gradients into the module's own parameters):
`pcd_backbone.forward` is re-bound on the instance and `remove()` restores it.  With training=True the gradients of the device fusion path flow into
the device backbone.

    accelerate(model, training=True, partition=True, backbone=True)

With `training=True, noising=True` the noising front end of the training branch (EXP/model.py:568-611) runs on the device as well:
`denoising_soft_procrustes.forward` is re-bound on the instance to the device fit under model.train() (the GT retry ladder's calls, :583; on its
0 / 1 matrices with more than K ones the reference's sort leaves the choice among equal entries unspecified and the device takes the lowest flat
indices -- parity-unpinned); the warp under model.train() is masked fill -> Sinkhorn -> top-K Procrustes -> R_forwd s + t_forwd as one autograd
chain, and the denoising transformer computes its point embedding with gradients enabled, so d loss / d denoising_coarse_matching.bin_score
carries the term through the warp that the reference has (without the flag the device path treats the warped points as constants); `q_sample`
is re-bound in the globals of the model's defining module to a version with cached schedule tables (bit-equal).  `remove()` restores every site.

    accelerate(model, training=True, partition=True, backbone=True, noising=True);  accelerate_loss(loss_fn, fine=True)

With `front=True` (any combination of the flags above) the geometry head of forward (EXP/model.py:302-351) runs on the device
(diffreg_hip/front2d3d.py): `back_project`, `render` and `create_meshgrid` are re-bound in the globals of the model's defining module, like the
partition's names, and `back_project_depth` on the instance; `remove()` restores all four.  Without the flag none of them is touched.  The two
feature-layout calls (:374-375, :535-538) are inline `F.` code and take a one-line edit each ("Geometry head and feature layout").

    accelerate(model, front=True)

With `image_backbone=True` (any combination of the flags above) the image backbone's INFERENCE forward (`self.img_backbone(image, dino)`,
EXP/model.py:358-361; EXP/image_backbone.py:254-289) runs on the device (diffreg_hip/image_backbone2d3d.py: NHWC token rows, the implicit-GEMM
convolution and the row resample of csrc/conv2d.hip, the point backbone's GroupNorm entries): `img_backbone.forward` is re-bound on the instance and
`remove()` restores it.  Under model.train() or with gradients enabled the bound forward calls the module's own code unchanged.  The flag is
opt-in and defaults off.

    accelerate(model, image_backbone=True)

With `image_backbone_grad=True` (implies image_backbone=True) the device path also runs under model.train() and with gradients enabled, and its
backward (the convolution's two gradients, the resample's gather, the GroupNorm backward) fills the .grad of img_backbone's own parameters.

    accelerate(model, training=True, backbone=True, noising=True, image_backbone_grad=True)

With `dino=True` (any combination of the flags above) the frozen DINOv2 ViT-L/14 that produces `img_feats_x_dino` (EXP/model.py:354-358,
EXP/encoders.py:107-119: `self.encoder.dinov2_vitl14[0].forward_features`) runs on the device in the reference's own fp16 arithmetic
(diffreg_hip/vit2d3d.py, csrc/vit.hip: fp16 MFMA GEMMs with fp32 accumulation, an fp32 residual stream, fp16 flash attention):
`forward_features` is re-bound on the ViT instance and `remove()` restores it.  It runs in eval and in training, with or without gradients
enabled (the reference wraps the call in torch.no_grad() and the network is frozen).  A ViT the kernels do not cover (not fp16, SwiGLU, a head
dim other than 64, ...) raises NotImplementedError here, before any site is bound.  The flag is opt-in and defaults off.

    accelerate(model, dino=True)

With `depth_head=True` (any combination of the flags above) the decoder of Depth-Anything (`model.depth_model.depth_head`, a DPTHead:
depth_anything/dpt.py:103-136, reached through EXP/model.py:343-351) runs on the device in float32 (diffreg_hip/dpt2d3d.py: the implicit-GEMM
convolution with the pre-activation / two-addend epilogue, the transposed convolution as a GEMM with a pixel-shuffle store, the fused tail and the
row resample of csrc/conv2d.hip): `depth_head.forward` is re-bound on the instance and `remove()` restores it.  The device path runs in eval mode
under torch.no_grad() with CUDA float32 inputs of batch 1; otherwise the bound forward calls the module's own code unchanged.  The trailing
F.interpolate + relu of DPT_DINOv2.forward (dpt.py:163-164) and the host-side Resize transform stay as they are (depth_transform=True, below, moves
both).  A head the kernels do not cover
(use_clstoken, nclass > 1, batch norm, ...) raises NotImplementedError here, before any site is bound.  The flag is opt-in and defaults off.

    accelerate(model, depth_head=True)

With `depth_encoder=True` (any combination of the flags above) the float32 ViT-L/14 in front of that decoder (`model.depth_model.pretrained`, the
hub's DinoVisionTransformer: depth_anything/dpt.py:158 calls its get_intermediate_layers(x, 4, return_class_token=True)) runs on the device in
exact fp32 products (diffreg_hip/depth_encoder2d3d.py, csrc/vit_f32.hip: the float32 rows GEMM on the f32-input MFMA with the ViT's epilogues
fused, the float32 attention on the packed qkv rows, the final norm of each taken stream written by the same call): `get_intermediate_layers`
is re-bound on the ViT instance and `remove()` restores it.  The device path runs in eval mode under torch.no_grad() with a CUDA float32 batch;
otherwise the bound method calls the module's own code unchanged.  A ViT the kernels do not cover (not entirely float32, register tokens, SwiGLU, a
head dim other than 64, ...) raises NotImplementedError here, before any site is bound.  The flag is opt-in and defaults off.  With
depth_head=True as well, everything from the transformed image tensor to the depth map runs in the library.

    accelerate(model, depth_encoder=True, depth_head=True)

pyramid=dict(num_stages=4, voxel_size=0.025, search_radius=0.0625, neighbor_limits=[...]): the graph pyramid the point backbone reads (`points`,
`lengths`, `neighbors`, `subsampling`, `upsampling`) is built on the device (diffreg_hip/pyramid2d3d.py on csrc/collate.hip: vision3d's grid
subsampling bit for bit up to the order of a stage's points, its radius search index for index on those points) instead of on the data loader's CPU
workers by GraphPyramid2D3DRegistrationCollateFn.  `model.forward` is re-bound on the instance: a `data_dict` whose `points` is still the stacked
[N, 3] tensor of a pyramid-less collate (with `lengths`; one cloud when absent) gets the five lists before the model's own forward runs; a dict that
already carries the lists passes through untouched.  `remove()` restores `forward`.  A neighbour limit above 64 raises NotImplementedError here,
before any site is bound.  The limits themselves come from pyramid2d3d.calibrate_neighbors_pack_mode, which needs no compiled vision3d extension
either.  The flag is opt-in (default None) and combines with every other flag.

    accelerate(model, backbone=True, pyramid=dict(num_stages=4, voxel_size=0.025, search_radius=0.0625, neighbor_limits=limits))

With `depth_transform=True` (implies depth_encoder=True, depth_head=True; any combination of the flags above) the input transform in front of
Depth-Anything (EXP/model.py:339-342: the device-to-host copy, Resize with cv2.INTER_CUBIC, NormalizeImage, PrepareForNet, the copy back) runs on
the device as one launch (diffreg_hip/depth_transform2d3d.py, csrc/image_transform.hip) and the whole depth branch becomes one engine
(diffreg_hip/depth_branch2d3d.py), in eval and in train mode, under its own torch.no_grad().  Three sites are re-bound: `model.forward` on the
instance stashes `data_dict["image"]` (composed with the pyramid's wrapper when both are set); `model.transform` on the instance returns
`{"image": <zero-size float32 ndarray>}` while an image is stashed; `predict_depth` in the globals of the model's defining module runs the engine
on the stashed device image when that zero-size image arrives and calls the original `predict_depth` on a real image.  `remove()` restores all
three.  In an unmodified file the inline `image.squeeze(0).squeeze(0).cpu().numpy()` of line 339 still executes, so ONE device-to-host copy (and
its stream drain) remains; the one-line edit of model.py:339-342 that calls `model._dr_overlay.depth(image)` removes it.
`depth_transform=dict(graph=True)` replays the branch as one captured graph (the depth map is then the graph's static output, valid until the next
forward); other keys of the dict go to DeviceTransform.  The flag is opt-in and defaults off.

    accelerate(model, depth_transform=True)

What then stays the reference's code in a training step: the encoder's CNN
branch (`encoder.cnn`, whose outputs MATR2D3D.forward discards) and `dino_2_u`, the inline GT retry ladder and the other inline glue of
MATR2D3D.forward.
"""
import sys
import types

import torch

from . import autograd2d3d, pcd_backbone2d3d
from .engine import DenoiseEngine2D3D


class LoopOverlay2D3D:
    def __init__(self, model, n_head=4, engine_kwargs=None, training=False, partition=False, backbone=False, noising=False, front=False,
                 image_backbone=False, image_backbone_grad=False, dino=False, depth_head=False, depth_encoder=False, pyramid=None,
                 depth_transform=False):
        self.model = model
        self._attr_saved = []
        self.depth_transform = depth_transform is not None and depth_transform is not False
        self.depth_branch, self._depth_image = None, None
        if self.depth_transform:            # first: a transform that cannot be built raises here, before any site is bound
            from .depth_transform2d3d import DeviceTransform
            opts = dict(depth_transform) if isinstance(depth_transform, dict) else {}
            self._depth_graph = bool(opts.pop("graph", False))
            self._depth_device_transform = DeviceTransform(**opts)
            depth_head = depth_encoder = True
        self.pyramid = None
        if pyramid is not None:             # first: a neighbour limit above 64 raises NotImplementedError here, before any site is bound
            from . import pyramid2d3d
            self.pyramid = pyramid2d3d.GraphPyramid2D3DCollate(**pyramid)
        self.dino = bool(dino)
        self.depth_head = bool(depth_head)
        self.depth_encoder = bool(depth_encoder)
        self.training = bool(training)
        self.partition = bool(partition)
        self.backbone = bool(backbone)
        self.noising = bool(noising)
        self.front = bool(front)
        self.image_backbone_grad = bool(image_backbone_grad)
        self.image_backbone = bool(image_backbone) or self.image_backbone_grad
        if self.noising and not self.training:
            raise ValueError("noising=True is the training branch's front end: it needs training=True")
        if self.image_backbone:             # first: a module without a device form raises NotImplementedError here, before any site is bound
            from . import image_backbone2d3d
            self.image_backbone_device = image_backbone2d3d.bind(model.img_backbone, grad=self.image_backbone_grad)
        if self.dino:                       # likewise: refuses before any site is bound
            from . import vit2d3d
            self.dino_binding = vit2d3d.bind(model.encoder)
        if self.depth_head:                 # likewise
            from . import dpt2d3d
            self.depth_head_undo = dpt2d3d.bind(model.depth_model.depth_head)
        if self.depth_encoder:              # likewise (a refusal here takes an already bound depth head back off)
            from . import depth_encoder2d3d
            try:
                self.depth_encoder_undo = depth_encoder2d3d.bind(model.depth_model)
            except NotImplementedError:
                self._unbind_front_modules()
                raise
        if self.depth_transform:            # both are bound: the engine reuses them and has nothing left to refuse
            from .depth_branch2d3d import DepthBranch2D3D
            self.depth_branch = DepthBranch2D3D(model.depth_model, transform=self._depth_device_transform)
        self._globals_saved = {}
        self.n_head = n_head
        self.engine_kwargs = dict(engine_kwargs or {})
        self.engine = None
        self._k = 0                 # step inside the current eval forward
        self._rec = {}
        self._out = None
        t, m = model.denoising_transformer, model.denoising_coarse_matching
        self._orig = dict(warp=model.get_warped_from_noising_matching3D3D, transformer=t.forward, matching=m.forward)
        model.get_warped_from_noising_matching3D3D = self._warp
        t.forward = self._transformer
        m.forward = self._matching
        if self.training:
            self._orig.update(coarse_transformer=model.transformer.forward, coarse_matching=model.coarse_matching.forward)
            model.transformer.forward = self._coarse_transformer
            model.coarse_matching.forward = self._coarse_matching
        if self.partition:
            self._bind_partition()
        if self.backbone:
            pb = model.pcd_backbone
            pb.forward = lambda feats, data_dict: pcd_backbone2d3d.point_backbone(pb, feats, data_dict)
        if self.noising:
            self._orig.update(procrustes=model.denoising_soft_procrustes.forward)
            model.denoising_soft_procrustes.forward = self._procrustes
            self._bind_globals({"q_sample": autograd2d3d.q_sample})
        if self.front:
            from . import front2d3d as f
            self._bind_globals({name: getattr(f, name) for name in ("back_project", "render", "create_meshgrid")})
            model.back_project_depth = f.back_project_depth
        if self.pyramid is not None or self.depth_transform:
            self._orig.update(forward=model.forward)
            self._bind_attr(model, "forward", self._forward)
        if self.depth_transform:
            self._orig.update(transform=model.transform)
            self._bind_attr(model, "transform", self._transform)
            self._bind_globals({"predict_depth": self._predict_depth})
        model._dr_overlay = self

    _MISSING = object()

    def _forward(self, data_dict, *args, **kwargs):
        """pyramid=...: a dict whose `points` is still the stacked [N, 3] tensor of a pyramid-less collate gets the five lists here, on the device;
        a dict that already carries the lists passes through untouched"""
        if self.pyramid is not None and torch.is_tensor(data_dict.get("points")):
            self.pyramid(data_dict)
        if not self.depth_transform:
            return self._orig["forward"](data_dict, *args, **kwargs)
        self._depth_image = self._device_image(data_dict.get("image"))       # depth_transform: what the depth branch of this forward reads
        try:
            return self._orig["forward"](data_dict, *args, **kwargs)
        finally:
            self._depth_image = None

    # ---- depth_transform: the three sites of EXP/model.py:339-342 ----------------------------------------------------------------------------
    @staticmethod
    def _device_image(image):
        """data_dict["image"] ([1, H, W, 3] on the device) as the [H, W, 3] view the transform reads, or None when it is anything else"""
        if not (torch.is_tensor(image) and image.is_cuda and image.dtype == torch.float32 and image.dim() >= 3 and image.shape[-1] == 3):
            return None
        if any(n != 1 for n in image.shape[:-3]):
            return None
        return image.detach().reshape(image.shape[-3:])

    def depth(self, image):
        """the depth map [1, h, w] of a device image ([H, W, 3] behind any number of leading 1s): what `predict_depth(self.depth_model,
        transform(image))` returns, with no host copy (INTEGRATION.md gives the one-line edit of model.py:339-342 that calls this)"""
        img = self._device_image(image)
        if img is None:
            raise TypeError("overlay depth: a CUDA float32 [..., H, W, 3] tensor with leading dimensions of 1; there is no CPU path")
        return self.depth_branch(img, graph=self._depth_graph)

    def _transform(self, sample):
        """model.transform: with a device image stashed by forward the host transform has nothing to do (a zero-size image goes through
        torch.from_numpy(...).unsqueeze(0).cuda() and tells _predict_depth to read the stash); anything else is the reference's own transform"""
        if self._depth_image is not None:
            import numpy as np
            return {"image": np.zeros((3, 0, 0), dtype=np.float32)}
        return self._orig["transform"](sample)

    def _predict_depth(self, depth_model, image):
        """predict_depth in the model's globals: the engine on the stashed device image (eval or train mode, under its own no_grad) when the
        zero-size image of _transform arrives; the original predict_depth on a real image"""
        if self._depth_image is not None and depth_model is self.model.depth_model and torch.is_tensor(image) and image.numel() == 0:
            return self.depth_branch(self._depth_image, graph=self._depth_graph)
        orig = self._globals_saved.get("predict_depth", self._MISSING)
        if orig is self._MISSING:
            with torch.no_grad():
                return depth_model(image)
        return orig(depth_model, image)

    def _unbind_front_modules(self):
        """a later bind refused: take off what the earlier flags of this constructor bound, so that a refusal leaves no site bound"""
        if self.image_backbone:
            self.model.img_backbone.__dict__.pop("forward", None)
        if self.dino:
            self.dino_binding.remove()
        if self.depth_head:
            self.depth_head_undo()

    def _bind_partition(self):
        """re-bind the module-level functions of EXP/model.py:395-540 (and, with training, :569) in the globals of the model's defining module"""
        from . import partition2d3d as p
        names = ["point_to_node_partition", "patchify", "get_2d3d_node_correspondences"]
        if self.training:
            names += ["get_correspondences", "to_o3d_pcd"]
        self._bind_globals({name: getattr(p, name) for name in names})

    def _bind_attr(self, obj, name, value):
        """set an instance attribute and remember what the instance's own __dict__ held before (nothing, for a method of the class)"""
        self._attr_saved.append((obj, name, obj.__dict__.get(name, self._MISSING)))
        setattr(obj, name, value)

    def _bind_globals(self, table):
        g = vars(sys.modules[type(self.model).__module__])
        for name, fn in table.items():
            self._globals_saved[name] = g.get(name, self._MISSING)
            g[name] = fn

    def remove(self):
        """restore every site this overlay bound: the instance attributes and the globals of the model's defining module"""
        m = self.model
        sites = [(m, "get_warped_from_noising_matching3D3D"), (m.denoising_transformer, "forward"), (m.denoising_coarse_matching, "forward")]
        if self.training:
            sites += [(m.transformer, "forward"), (m.coarse_matching, "forward")]
        if self.backbone:
            sites += [(m.pcd_backbone, "forward")]
        if self.noising:
            sites += [(m.denoising_soft_procrustes, "forward")]
        if self.front:
            sites += [(m, "back_project_depth")]
        if self.image_backbone:
            sites += [(m.img_backbone, "forward")]
        if self.depth_branch is not None:    # (binds nothing of its own here: the two flags above did; this drops its graphs)
            self.depth_branch.remove()
        if self.dino:
            self.dino_binding.remove()
        if self.depth_head:
            self.depth_head_undo()
        if self.depth_encoder:
            self.depth_encoder_undo()
        for obj, name in sites:
            if name in obj.__dict__:
                del obj.__dict__[name]
        for obj, name, old in reversed(self._attr_saved):
            if old is self._MISSING:
                obj.__dict__.pop(name, None)
            else:
                obj.__dict__[name] = old
        self._attr_saved = []
        if self._globals_saved:
            g = vars(sys.modules[type(m).__module__])
            for name, old in self._globals_saved.items():
                if old is self._MISSING:
                    g.pop(name, None)
                else:
                    g[name] = old
            self._globals_saved = {}
        m.__dict__.pop("_dr_overlay", None)

    def refresh(self):
        """call after the weights changed (load_state_dict, .to()): the engine holds its own device copy"""
        self.engine = None
        if self.depth_branch is not None:
            self.depth_branch.refresh()

    # ---- engine from the model's own weights and hyper-parameters ------------------------------------------------------------
    def _build(self, device):
        sd = {k: v for k, v in self.model.state_dict().items() if k.startswith("denoising_transformer.") or k.startswith("denoising_coarse_matching.")}
        p = "denoising_transformer."
        n_layers = 1 + max(int(k[len(p + "transformer."):].split(".")[0]) for k in sd if k.startswith(p + "transformer."))
        proc, match = self.model.denoising_soft_procrustes, self.model.denoising_coarse_matching
        try:                                 # vision3d TransformerLayer -> AttentionLayer -> MultiHeadAttention.num_heads (vision3d/layers/transformer.py:29)
            self.n_head = int(self.model.denoising_transformer.transformer[0].attention.attention.num_heads)
        except (AttributeError, IndexError, TypeError):
            pass
        kw = dict(C=sd[p + "out_proj.weight"].shape[0], H=self.n_head, n_layers=n_layers, img_dim=sd[p + "img_in_proj.weight"].shape[1],
                  dino_dim=sd[p + "img_in_proj_dino.weight"].shape[1], pcd_dim=sd[p + "pcd_in_proj.weight"].shape[1],
                  steps=int(self.model.sampling_timesteps), sk_iters=int(match.skh_iters), sample_rate=float(proc.sample_rate),
                  max_condition_num=float(proc.max_condition_num), device=device)
        kw.update(self.engine_kwargs)
        self.engine = DenoiseEngine2D3D(sd, **kw)

    # ---- the three call sites ------------------------------------------------------------------------------------------------
    def _warp(self, s_pcd, t_pcd, src_mask, tgt_mask, matrix):
        if self.model.training:
            if self.noising and src_mask is not None:      # (without masks the reference's own code raises: conf is never assigned, :832-841)
                return autograd2d3d.noising_warp(self.model, s_pcd, t_pcd, src_mask, tgt_mask, matrix)
            return self._orig["warp"](s_pcd, t_pcd, src_mask, tgt_mask, matrix)
        if self._k == 0:
            self._rec = dict(s_pcd=s_pcd, t_pcd_da=t_pcd, src_mask=src_mask, tgt_mask_da=tgt_mask, x_T=matrix.detach().clone())
            self._out = None
        if src_mask is not None:            # the reference masks x IN PLACE here (:832-834) and the -inf entries persist in its x
            matrix.masked_fill_(~(src_mask[..., None] * tgt_mask[:, None]).bool(), float("-inf"))
        if self._out is not None:           # steps >= 1: this step's warp from the device trace
            Rf, tf = self._out["R_forwd"][self._k], self._out["t_forwd"][self._k]
            return (torch.matmul(Rf, s_pcd.transpose(1, 2)) + tf).transpose(1, 2), t_pcd.type(torch.float32), Rf, tf
        # step 0: the loop has not run yet (its remaining inputs arrive with the next two calls); nothing on this path reads these
        eye = torch.eye(3, device=s_pcd.device)[None].expand(s_pcd.shape[0], 3, 3)
        return s_pcd.type(torch.float32), t_pcd.type(torch.float32), eye, torch.zeros(s_pcd.shape[0], 3, 1, device=s_pcd.device)

    def _transformer(self, img_feats, img_dino, img_pixels, pcd_feats, pcd_points):
        if self.model.training:
            if self.training:
                return autograd2d3d.fusion_module(self.model.denoising_transformer, img_feats, img_dino, img_pixels, pcd_feats, pcd_points,
                                                  embed_grad=self.noising)
            return self._orig["transformer"](img_feats, img_dino, img_pixels, pcd_feats, pcd_points)
        if self._k == 0:
            self._rec.update(img_feats=img_feats, img_dino=img_dino, img_pixels=img_pixels, pcd_feats=pcd_feats)
        if self._out is not None:           # the fused features of the LAST step (the loop keeps no others)
            return self._out["img_feats"], self._out["pcd_feats"]
        return img_feats, pcd_feats         # step 0 placeholders, consumed by the matching call below only

    def _matching(self, src_feats, tgt_feats, src_mask, tgt_mask, *args, **kwargs):
        if self.model.training:
            if self.training:
                return autograd2d3d.matching_head_2d3d(self.model.denoising_coarse_matching, src_feats, tgt_feats, src_mask, tgt_mask, *args, **kwargs)
            return self._orig["matching"](src_feats, tgt_feats, src_mask, tgt_mask, *args, **kwargs)
        if self._k == 0:
            r = self._rec
            dev = r["s_pcd"].device
            if self.engine is None or self.engine.device != dev:
                self._build(dev)
            masks = None if src_mask is None else (src_mask, tgt_mask, r["tgt_mask_da"])
            f = lambda t_: t_.detach().float()
            self._out = self.engine.run(f(r["img_feats"]), f(r["img_dino"]), f(r["img_pixels"]), f(r["pcd_feats"]), f(r["s_pcd"]), f(r["t_pcd_da"]),
                                        f(r["x_T"]), masks, trace=True)
        x_start = self._out["x0"][self._k]
        self._k += 1
        if self._k >= self.engine.steps:
            self._k = 0
            self._rec = {}
        return x_start, None, None, None


    def _procrustes(self, conf_matrix, src_pcd, tgt_pcd, src_mask, tgt_mask):
        if self.model.training:
            return autograd2d3d.soft_procrustes(self.model.denoising_soft_procrustes, conf_matrix, src_pcd, tgt_pcd, src_mask, tgt_mask)
        return self._orig["procrustes"](conf_matrix, src_pcd, tgt_pcd, src_mask, tgt_mask)

    # ---- the training branch's coarse modules (training=True): the device path in train mode, the original code in eval mode ---------------
    def _coarse_transformer(self, img_feats, img_dino, img_pixels, pcd_feats, pcd_points, *args, **kwargs):
        if self.model.training and not args and not kwargs:
            return autograd2d3d.fusion_module(self.model.transformer, img_feats, img_dino, img_pixels, pcd_feats, pcd_points)
        return self._orig["coarse_transformer"](img_feats, img_dino, img_pixels, pcd_feats, pcd_points, *args, **kwargs)

    def _coarse_matching(self, src_feats, tgt_feats, src_mask, tgt_mask, *args, **kwargs):
        if self.model.training:
            return autograd2d3d.matching_head_2d3d(self.model.coarse_matching, src_feats, tgt_feats, src_mask, tgt_mask, *args, **kwargs)
        return self._orig["coarse_matching"](src_feats, tgt_feats, src_mask, tgt_mask, *args, **kwargs)


def accelerate(model, n_head=4, training=False, partition=False, backbone=False, noising=False, front=False, image_backbone=False,
               image_backbone_grad=False, dino=False, depth_head=False, depth_encoder=False, pyramid=None, depth_transform=False,
               **engine_kwargs):
    """install the overlay on a MATR2D3D instance (see the module docstring); returns the LoopOverlay2D3D (`.remove()` undoes it).
    training=True: the training branch's four coarse modules run on the device under model.train() as well.
    partition=True: the patch partition and GT patch overlaps (and, with training, the GT search) run on the device as well.
    backbone=True: the point backbone (model.pcd_backbone) runs on the device, in eval and train mode.
    noising=True (with training=True): the GT ladder's Procrustes fits, q_sample and the warp run on the device under model.train(), and the
    warp's gradient reaches denoising_coarse_matching.bin_score.
    front=True: back_project, render, create_meshgrid (globals of the model's module) and back_project_depth (the instance) run on the device.
    image_backbone=True: model.img_backbone's inference forward runs on the device (eval mode under torch.no_grad(); otherwise its own code).
    image_backbone_grad=True (implies image_backbone): the device path also runs in training mode and with gradients enabled, with its backward.
    dino=True: the frozen DINOv2 ViT of model.encoder (dinov2_vitl14[0].forward_features) runs on the device in fp16, in eval and in training.
    depth_head=True: model.depth_model.depth_head (Depth-Anything's DPT decoder) runs on the device in float32 (eval mode under torch.no_grad();
    otherwise its own code).
    depth_encoder=True: model.depth_model.pretrained.get_intermediate_layers (Depth-Anything's float32 ViT-L/14) runs on the device in exact fp32
    products (eval mode under torch.no_grad() with a CUDA float32 batch; otherwise its own code).
    pyramid=dict(num_stages=, voxel_size=, search_radius=, neighbor_limits=): model.forward builds the graph pyramid on the device when
    data_dict["points"] is the stacked tensor of a pyramid-less collate (diffreg_hip/pyramid2d3d.py); None (the default) touches nothing.
    depth_transform=True (implies depth_encoder and depth_head): Depth-Anything's input transform runs on the device and the depth branch reads
    data_dict["image"] where it lies (diffreg_hip/depth_branch2d3d.py); depth_transform=dict(graph=True) replays the branch as one captured graph
    (other keys go to DeviceTransform)."""
    return LoopOverlay2D3D(model, n_head=n_head, engine_kwargs=engine_kwargs, training=training, partition=partition, backbone=backbone,
                           noising=noising, front=front, image_backbone=image_backbone, image_backbone_grad=image_backbone_grad,
                           dino=dino, depth_head=depth_head, depth_encoder=depth_encoder, pyramid=pyramid, depth_transform=depth_transform)


def accelerate_loss(loss_module, fine=False):
    """re-bind CoarseMatchingLoss.forward of `loss_module` (or of its `c_loss`: an OverallLoss) to autograd2d3d.coarse_matching_loss, on the
    instance; fine=True: also FineMatchingLoss.forward of its `f_loss` to autograd2d3d.fine_matching_loss.  Returns a function that restores
    every site it bound."""
    if fine and not hasattr(loss_module, "f_loss"):          # (before anything is bound)
        raise ValueError("accelerate_loss(fine=True) needs an OverallLoss (a module with c_loss and f_loss)")
    target = loss_module.c_loss if hasattr(loss_module, "c_loss") else loss_module
    target.forward = lambda output_dict: autograd2d3d.coarse_matching_loss(target, output_dict)
    bound = [target]
    if fine:
        f = loss_module.f_loss
        f.forward = lambda data_dict, output_dict: autograd2d3d.fine_matching_loss(f, data_dict, output_dict)
        bound.append(f)

    def restore():
        for mod in bound:
            mod.__dict__.pop("forward", None)
    return restore
