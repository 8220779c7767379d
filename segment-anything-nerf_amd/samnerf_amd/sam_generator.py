"""SAM's automatic mask generator over a rendered feature map, on the device
(csrc/sam_decoder.hip, include/samnerf_hip.h "prompt batches"): the point
grid decoded in chunks by SamDecoder.decode_batch, the predicted-IoU and
stability filters and the boxes by mask_stats (no logit image is written),
one greedy box NMS, one masks_select of the kept masks, one host read.

One crop equal to the image only.  Not built, each a NotImplementedError:
crop_n_layers > 0 (a crop needs the ViT on the cropped image),
min_mask_region_area > 0 (OpenCV's connected components) and the RLE output
modes.
"""
import numpy as np
import torch

from .sam_decoder import MAX_CANDIDATES, MAX_SETS, REC_WORDS

REC_FIELDS = ("inter", "union", "area", "x0", "y0", "x1", "y1", "stability", "pass", "iou")


def build_point_grid(n_per_side):
    """An n x n grid of points in [0, 1]^2, (x, y) rows, x fastest: (i + 0.5) / n."""
    offset = 1 / (2 * n_per_side)
    side = np.linspace(offset, 1 - offset, n_per_side)
    xs = np.tile(side[None, :], (n_per_side, 1))
    ys = np.tile(side[:, None], (1, n_per_side))
    return np.stack([xs, ys], axis=-1).reshape(-1, 2)


def input_size_for(H, W, S):
    r = S / W if W > H else S / H
    return int(H * r), int(W * r)


class DeviceMaskGenerator:
    def __init__(self, decoder, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88,
                 stability_score_thresh=0.95, stability_score_offset=1.0, box_nms_thresh=0.7, max_masks=256,
                 crop_n_layers=0, min_mask_region_area=0, output_mode="binary_mask", mask_threshold=0.0):
        if crop_n_layers > 0:
            raise NotImplementedError("DeviceMaskGenerator: crop_n_layers > 0 is not built (a crop needs the ViT "
                                      "image encoder on the cropped image)")
        if min_mask_region_area > 0:
            raise NotImplementedError("DeviceMaskGenerator: min_mask_region_area > 0 is not built (small-region "
                                      "removal is OpenCV's connected components)")
        if output_mode != "binary_mask":
            raise NotImplementedError(f"DeviceMaskGenerator: output_mode {output_mode!r} is not built (the RLE "
                                      "modes 'uncompressed_rle' and 'coco_rle'); 'binary_mask' only")
        if not 1 <= points_per_batch <= MAX_SETS:
            raise ValueError(f"DeviceMaskGenerator: points_per_batch must lie in [1, {MAX_SETS}]")
        if not 1 <= points_per_side or 3 * points_per_side ** 2 > MAX_CANDIDATES:
            raise ValueError("DeviceMaskGenerator: points_per_side must lie in [1, 64]")
        if max_masks < 1:
            raise ValueError("DeviceMaskGenerator: max_masks must be at least 1")
        self.decoder = decoder
        self.points_per_side, self.points_per_batch = int(points_per_side), int(points_per_batch)
        self.pred_iou_thresh, self.stability_score_thresh = float(pred_iou_thresh), float(stability_score_thresh)
        self.stability_score_offset, self.box_nms_thresh = float(stability_score_offset), float(box_nms_thresh)
        self.mask_threshold, self.max_masks = float(mask_threshold), int(max_masks)
        self.point_grid = build_point_grid(self.points_per_side)
        self.truncated = None
        self._points = {}

    def points_for(self, H, W):
        """(the grid in the view's frame [n, 2] float64, the same in the
        decoder's input frame): SamAutomaticMaskGenerator's points_for_image
        and ResizeLongestSide.apply_coords."""
        in_h, in_w = input_size_for(H, W, self.decoder.S)
        pts = self.point_grid * np.array([[W, H]], dtype=np.float64)
        return pts, pts * np.array([[in_w / W, in_h / H]])

    def generate(self, features, H, W, multimask_output=True, as_tensors=False):
        """features: the image tokens [g*g, 256] or a rendered map [h, w, 256]
        on the device.  Returns the list of mask records in NMS order (dicts of
        segmentation, a bool [H, W] view of the device's mask table; area;
        bbox XYWH; predicted_iou; point_coords; stability_score; crop_box), at
        most max_masks of them (`truncated` says whether more were kept).
        as_tensors=True returns the device tensors instead and reads nothing
        back: dict(masks [cap, H, W] bool, records [cap, REC_WORDS] int32 of
        the kept candidates in order, keep [n], count [1], points)."""
        dec = self.decoder
        H, W = int(H), int(W)
        size, L = input_size_for(H, W, dec.S), 4 * dec.g
        pts_view, pts_in = self.points_for(H, W)
        n_pts, M = len(pts_in), 3 if multimask_output else 1
        sel = slice(1, 4) if multimask_output else slice(0, 1)
        n = n_pts * M                                      # candidate = point * M + mask: flatten(0, 1)
        dev = dec.device
        if (H, W) not in self._points:                     # the grid goes up once per view size
            self._points[H, W] = torch.as_tensor(pts_in.astype(np.float32)).to(dev).view(n_pts, 1, 2)
        points = self._points[H, W]
        low = torch.empty(n, L, L, device=dev)
        iou = torch.empty(n, device=dev)
        records = torch.empty(n, REC_WORDS, dtype=torch.int32, device=dev)
        for p0 in range(0, n_pts, self.points_per_batch):             # the last chunk is ragged
            p1 = min(p0 + self.points_per_batch, n_pts)
            lo, io = dec.decode_batch(features, points[p0:p1])
            c0, c1 = p0 * M, p1 * M
            low[c0:c1] = lo[:, sel].reshape(c1 - c0, L, L)
            iou[c0:c1] = io[:, sel].reshape(c1 - c0)
            dec.mask_stats(low[c0:c1], iou[c0:c1], size, (H, W), self.pred_iou_thresh,
                           self.stability_score_thresh, self.stability_score_offset, self.mask_threshold,
                           out=records[c0:c1])
        # With one crop equal to the image the reference's is_box_near_crop_edge filter removes nothing: it
        # spares every box near the image's own edge, and here the crop's edge is that edge.
        keep, count = dec.nms(records, self.box_nms_thresh)
        cap = min(self.max_masks, n)
        masks = dec.masks_select(low, size, (H, W), index=keep, count=count, cap=cap,
                                 mask_threshold=self.mask_threshold)
        kept = records[keep[:cap].clamp(min=0).long()]
        if as_tensors:
            return dict(masks=masks, records=kept, keep=keep, count=count, points=points)
        host = torch.cat([count, keep[:cap], kept.reshape(-1)]).cpu().numpy()      # the one host read
        total, keep_h, rec = int(host[0]), host[1:1 + cap], host[1 + cap:].reshape(cap, REC_WORDS)
        self.truncated = total > cap
        rec_f = rec.view(np.float32)
        out = []
        for i in range(min(total, cap)):
            r, c = rec[i], int(keep_h[i])
            x0, y0, x1, y1 = (int(v) for v in r[3:7])
            out.append(dict(segmentation=masks[i], area=int(r[2]), bbox=[x0, y0, x1 - x0, y1 - y0],
                            predicted_iou=float(rec_f[i, 9]), point_coords=[pts_view[c // M].tolist()],
                            stability_score=float(rec_f[i, 7]), crop_box=[0, 0, W, H], candidate=c))
        return out
