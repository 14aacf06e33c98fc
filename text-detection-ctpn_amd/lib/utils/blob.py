"""im_list_to_blob with the reference's contract (lib/utils/blob.py:6-19): zero-padded NHWC float32 batch."""
import numpy as np


def im_list_to_blob(ims):
    shapes = np.array([im.shape for im in ims])
    hmax, wmax = int(shapes[:, 0].max()), int(shapes[:, 1].max())
    blob = np.zeros((len(ims), hmax, wmax, 3), dtype=np.float32)
    for i, im in enumerate(ims):
        blob[i, :im.shape[0], :im.shape[1], :] = im
    return blob


def im_list_to_canvas(ims):
    """Images of ONE width and different heights -> (canvas, heights) of a ragged batch (Context.forward_ragged / detect_ragged):
    canvas (n, max height, w, 3) uint8, image i in rows [0, heights[i]) of slot i, zeros below it (any bytes would do: they are never read
    as pixels); heights int32. Mixed widths are an error: group by width first."""
    if not len(ims):
        raise ValueError("im_list_to_canvas: no images")
    w = ims[0].shape[1]
    if any(im.ndim != 3 or im.shape[2] != 3 or im.shape[1] != w for im in ims):
        raise ValueError("im_list_to_canvas: images must be (h, w, 3) of one width")
    heights = np.array([im.shape[0] for im in ims], np.int32)
    canvas = np.zeros((len(ims), int(heights.max()), w, 3), dtype=np.uint8)
    for i, im in enumerate(ims):
        canvas[i, :im.shape[0]] = im
    return canvas, heights
