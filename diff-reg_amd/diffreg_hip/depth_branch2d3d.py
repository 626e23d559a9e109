"""The depth branch of the 2D-3D front end as one engine: image on the device -> input transform -> ViT encoder -> DPT head -> depth map, with no
host read in between.

EXP/model.py:339-342 is `predict_depth(self.depth_model, transform(image))` with the transform on the host.  DepthBranch2D3D runs the transform as
one launch (diffreg_hip/depth_transform2d3d.py) in front of the device encoder (depth_encoder2d3d.bind) and the device head (dpt2d3d.bind), which
it binds itself unless they are bound already, and returns what predict_depth returns:

    branch = DepthBranch2D3D(model.depth_model)            # NotImplementedError for what the encoder or the head refuse, nothing left bound
    depth = branch(image_hwc)                              # CUDA float32 [H, W, 3] -> [1, h, w]
    depth = branch(image_hwc, graph=True)                  # the same values from a captured graph (see __call__ for the lifetime of the result)

DPT_DINOv2.forward ends in F.interpolate(size=(h, w), align_corners=True) and F.relu (depth_anything/dpt.py:163-164).  The transform makes h and w
multiples of 14, so (h, w) == (14 patch_h, 14 patch_w): a same-size align_corners=True resample is the identity and the head already ends in a
ReLU, so the two are skipped and the result is torch.equal to the unskipped path.  For any other size both run as in the reference.
"""
import collections

import torch
import torch.nn.functional as F

from . import depth_encoder2d3d, dpt2d3d
from .depth_transform2d3d import DeviceTransform

MAX_GRAPHS = 4


class _Captured:
    def __init__(self, static_in, graph, out):
        self.static_in, self.graph, self.out = static_in, graph, out


class DepthBranch2D3D:
    def __init__(self, depth_model, transform=None):
        self.depth_model = depth_model
        self.transform = transform if transform is not None else DeviceTransform()
        self._undo = []
        self._graphs = collections.OrderedDict()
        vit, head = depth_model.pretrained, depth_model.depth_head
        try:                                 # an encoder / head that is bound already (the overlay's flags, another engine) is reused as it is
            if "get_intermediate_layers" not in vit.__dict__:
                self._undo.append(depth_encoder2d3d.bind(depth_model))
            if "forward" not in head.__dict__:
                self._undo.append(dpt2d3d.bind(head))
        except NotImplementedError:
            self.remove()
            raise

    def remove(self):
        """undo what this object itself bound (an encoder or head that was bound before stays bound) and drop the graphs"""
        self._graphs.clear()
        while self._undo:
            self._undo.pop()()

    def refresh(self):
        """call after the weights changed: a captured graph reads the packed weight images of its capture"""
        self._graphs.clear()

    @property
    def graphs(self):
        """the source shapes that hold a captured graph, oldest first"""
        return [key[0] for key in self._graphs]

    def _depth(self, x):
        """DPT_DINOv2.forward on x [1, 3, h, w] without its trailing same-size resample + ReLU"""
        dm = self.depth_model
        h, w = x.shape[-2:]
        ph, pw = h // 14, w // 14
        feats = dm.pretrained.get_intermediate_layers(x, 4, return_class_token=True)
        depth = dm.depth_head(feats, ph, pw)
        if tuple(depth.shape[-2:]) != (h, w):
            depth = F.relu(F.interpolate(depth, size=(h, w), mode="bilinear", align_corners=True))
        return depth.squeeze(1)

    def _eager(self, image_hwc):
        return self._depth(self.transform(image_hwc))

    def _capture(self, image_hwc):
        static_in = torch.empty(tuple(image_hwc.shape), dtype=torch.float32, device=image_hwc.device)
        static_in.copy_(image_hwc)
        self._eager(static_in)                               # the position rows, the packed weights and the allocator's blocks, outside the capture
        torch.cuda.synchronize(image_hwc.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                        # one stream, no side streams: the graph has no parallel branches
            out = self._eager(static_in)
        return _Captured(static_in, graph, out)

    def __call__(self, image_hwc, graph=False):
        """image_hwc: CUDA float32 [H, W, 3] (TypeError otherwise) -> the depth map [1, h, w] = predict_depth(depth_model, transform(image)).

        graph=False: the transform launch followed by the depth model under torch.no_grad().
        graph=True: the first call for a source shape copies the image into a static buffer and captures transform -> encoder -> head into one
        torch.cuda.CUDAGraph; every call then copies the image into that buffer and replays.  THE RETURNED TENSOR IS THE GRAPH'S STATIC OUTPUT: it
        is valid until the next call of this object (which overwrites it) or until refresh() / remove() -- clone it to keep it.  A new source
        shape captures a new graph; at most MAX_GRAPHS are kept, the one used longest ago goes first.  After the weights changed call refresh()."""
        with torch.no_grad():
            if not graph:
                return self._eager(image_hwc)
            if not (torch.is_tensor(image_hwc) and image_hwc.is_cuda and image_hwc.dtype == torch.float32 and image_hwc.dim() == 3
                    and image_hwc.shape[2] == 3):
                raise TypeError("DepthBranch2D3D: a CUDA float32 [H, W, 3] tensor; there is no CPU path")
            key = (tuple(image_hwc.shape), image_hwc.device)
            with torch.cuda.device(image_hwc.device):
                ent = self._graphs.get(key)
                if ent is None:
                    ent = self._capture(image_hwc)
                    self._graphs[key] = ent
                    while len(self._graphs) > MAX_GRAPHS:
                        self._graphs.popitem(last=False)
                else:
                    self._graphs.move_to_end(key)
                    ent.static_in.copy_(image_hwc)
                ent.graph.replay()
            return ent.out
