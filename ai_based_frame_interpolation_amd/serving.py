"""Persistent in-process serving entry.

The reference's web API runs `python model/inference.py ...` as a SUBPROCESS for every request
(/root/reference/api/app.py:65-119 `run_inference`): each request pays a Python start-up, a
69 MB checkpoint load, a model build and a host->device copy before its single forward, and the
handler blocks on `subprocess.run` with a 300 s timeout.  `InterpolationService` keeps what that
subprocess rebuilds every time alive across requests:

  * the model with its prepared weights resident in HBM (uploaded once),
  * one workspace per frame shape,
  * one captured HIP graph per frame shape (`GraphedForward`: the reference's own 256x256 request
    is launch-bound, a replay is one launch),

and implements the same request contract -- two frames, `num_intermediate` (1-10), `fps` (10-60)
-> the frame list the reference writes to `video.mp4`: [frame1, N intermediates, frame2], all
post-processed to uint8 exactly as model/inference.py:main does (:262-291; the network has no
time input, so the N intermediates are identical: inference.py:141-147).  There is no web
framework here: an HTTP layer (FastAPI in the reference) would call `interpolate()` from its
handler and encode the returned frames; no codec is available in this image, so `save_frames`
writes the raw uint8 stack as `.npy`.

Requests are serialised by a lock (one HIP context, one stream): the reference isolates requests
by process, this class by mutual exclusion.
"""
from __future__ import annotations

import threading
import time
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _native
from .inference import load_model, preprocess_image
from .unet import FrameInterpolationUNet, GraphedForward

Frame = Union[str, np.ndarray]


class InterpolationService:
    """`svc = InterpolationService("best_model.pth"); frames = svc.interpolate(a, b, 3, 30)["frames"]`"""

    def __init__(self, model_path: Optional[str] = None, device: str = "cuda", precision: Optional[str] = None,
                 model: Optional[FrameInterpolationUNet] = None, target_size: Optional[Tuple[int, int]] = (256, 256),
                 use_graph: bool = True, weight_prep: Optional[str] = None):
        self.device = torch.device("cuda" if device in ("auto", None) else device)
        if self.device.type != "cuda":
            raise RuntimeError("InterpolationService (MI355X build) needs a HIP device; there is no CPU fallback")
        if model is not None and weight_prep is not None:
            # the service holds the caller's model, not a copy: like a plain `model.weight_prep = ...`, this is seen by
            # every other user of that model (outputs are the same either way); an invalid value leaves it as it was
            previous, model.weight_prep = model.weight_prep, weight_prep
            try:
                model._weight_prep_checked()
            except ValueError:
                model.weight_prep = previous
                raise
        self.model = model if model is not None else load_model(model_path, self.device, precision,
                                                                weight_prep=weight_prep)
        self.model.eval()
        self.target_size = target_size      # (width, height) like preprocess_image; None = keep size
        self.use_graph = use_graph
        self._graphs: Dict[Tuple[int, int, int], GraphedForward] = {}
        self._lock = threading.Lock()
        self.stats = {"requests": 0, "graph_captures": 0, "weight_uploads_seen": 0, "last_ms": 0.0}

    # ---- request validation: api/app.py:139-144 ------------------------------------------------
    @staticmethod
    def _validate(num_intermediate: int, fps: int):
        if num_intermediate < 1 or num_intermediate > 10:
            raise ValueError("num_intermediate must be between 1 and 10")
        if fps < 10 or fps > 60:
            raise ValueError("fps must be between 10 and 60")

    def _forward(self, f1: torch.Tensor, f2: torch.Tensor) -> torch.Tensor:
        if not self.use_graph:
            return self.model(f1, f2)
        key = tuple(f1.shape[1:]) + (f1.shape[0],)
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = GraphedForward(self.model, f1.shape[0], f1.shape[2], f1.shape[3])
        return g(f1, f2)

    def interpolate(self, frame1: Frame, frame2: Frame, num_intermediate: int = 3, fps: int = 30) -> dict:
        """One request.  frame1 / frame2: image paths (`.npy`, PGM/PPM, anything cv2 reads when it
        is installed) or decoded uint8 arrays.  Returns {"frames": [uint8 HxW arrays], "fps": fps,
        "num_frames": N + 2, "ms": wall time of this request}."""
        self._validate(num_intermediate, fps)
        t0 = time.perf_counter()
        with self._lock:
            t1 = preprocess_image(frame1, self.target_size).to(self.device)   # inference.py:228-229
            t2 = preprocess_image(frame2, self.target_size).to(self.device)
            if t1.shape != t2.shape:
                raise ValueError("the two frames must have the same size")
            mid = self._forward(t1, t2)                                      # inference.py:120
            # post-processing of all three distinct frames on device, one copy back
            stack = torch.cat([t1, mid, t2], dim=0)
            u8 = _native.postprocess_u8(stack.contiguous()).cpu().numpy()    # inference.py:54-61
            self.stats["requests"] += 1
            self.stats["graph_captures"] = sum(g.captures for g in self._graphs.values())
            self.stats["weight_uploads_seen"] = self.model._weights_gen
        frames: List[np.ndarray] = [u8[0, 0]] + [u8[1, 0]] * num_intermediate + [u8[2, 0]]
        ms = (time.perf_counter() - t0) * 1e3
        self.stats["last_ms"] = ms
        return {"frames": frames, "fps": fps, "num_frames": len(frames), "ms": ms}

    #: name of the function this replaces (api/app.py:65), same argument order
    run_inference = interpolate

    @staticmethod
    def save_frames(frames: List[np.ndarray], output_path: str, fps: int = 30) -> str:
        """Counterpart of save_frames_as_video (inference.py:176-202) without a codec: the uint8
        stack as `.npy` (frames) next to the frame rate."""
        arr = np.stack([f if f.dtype == np.uint8 else f.astype(np.uint8) for f in frames])
        if not output_path.endswith(".npy"):
            output_path += ".npy"
        np.save(output_path, arr)
        with open(output_path[:-4] + ".fps.txt", "w") as f:
            f.write(f"{fps}\n")
        return output_path
