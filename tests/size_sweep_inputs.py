"""The input sizes of the size sweep (tests/test_size_sweep_host.py on the CPU, tests/test_gpu_size_sweep.py on the GPU) and what
follows from a size alone: the net input the reference's rule makes of it (SCALES = (600,), MAX_SIZE = 1000 -- always through the
ORACLE's prep, never the product's), the chain of map sizes under the trunk's four ceil-mode poolings, the 13 trunk convolutions'
(H, W, Cin, Cout) and the anchor count.

Every other full-width comparison with the oracle runs at 600x1000 (scale exactly 1: the resize is the identity, the trunk sees
600x1000 -> 300x500 -> 150x250 -> 75x125 -> 38x63 and nothing else).  A VOC image is almost never that size; the entries below are
the sizes a VOC run really feeds, plus the edges of the rule (the MAX_SIZE cap, fewer anchors than the pre-NMS 6000, a scale above
2, a scale below 1).

SIZES is in RUN order: the net input's area goes up and down from one entry to the next (the context's scratch need is not
monotonic in it either: tests/test_gpu_pipeline.py::test_graph_is_dropped_when_a_context_arena_moves), so one net run down the
list meets smaller and larger buffers after each other, in both directions when the list is reversed."""
import numpy as np

from oracle import host as ohost

# (original h, original w, seed of the image's pixels)
SIZES = (
    (75, 500, 101),      # extreme landscape panorama: capped at MAX_SIZE -> 150x1000, 10x63 map, 5670 anchors < 6000
    (375, 500, 102),     # the commonest VOC shape -> 600x800
    (120, 100, 103),     # long side below 300 -> scale 6 -> 720x600
    (333, 500, 104),     # -> 600x901 (odd width)
    (500, 281, 105),     # portrait panorama, capped -> 1000x562 (the odd chain across the width: 281, 141, 71, 36)
    (500, 375, 106),     # -> 800x600
    (30, 500, 111),      # a strip -> 60x1000, 4x63 map, 2268 anchors: the oracle's ProposalLayer returns FEWER than 300 rois
    (281, 500, 107),     # odd VOC size AND landscape panorama, capped -> 562x1000: 281, 141, 71, 36 down the chain
    (500, 500, 108),     # -> 600x600
    (500, 333, 109),     # -> 901x600 (odd height)
    (1200, 1600, 110),   # larger than the net input: prep scales DOWN (0.5) -> 600x800, the trunk shapes of 375x500
)
UNDER_6000 = (75, 500)           # the entry the issue names: fewer anchors than RPN_PRE_NMS_TOP_N (the strip has fewer still)
FEW_ROIS = (30, 500)             # the entry with fewer rois than RPN_POST_NMS_TOP_N (tests/test_size_sweep_host.py records how many)
TRUNK_CHANNELS = (64, 128, 256, 512, 512)              # VGG-16 (models.write_mnc_5stage_test_prototxt() at full width)
TRUNK_LAYERS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3",
                "conv5_1", "conv5_2", "conv5_3")
TRUNK_STAGE = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
POOL_AFTER = ("conv1_2", "conv2_2", "conv3_3", "conv4_3")      # test.prototxt: pool1..pool4, MAX 2x2/2, Caffe's ceil output size
NUM_ANCHORS = 9


def image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def net_input(h, w):
    """-> (net input height, width, scale) by the oracle's prep (the content of the image plays no part in the geometry)."""
    data, im_info, scale = ohost.prepare_mnc_args(np.zeros((h, w, 3), np.uint8))
    assert im_info[0, 0] == data.shape[2] and im_info[0, 1] == data.shape[3]
    return int(data.shape[2]), int(data.shape[3]), float(scale)


def pool_out(n):
    """Caffe's Pooling output size for kernel 2 stride 2 pad 0: ceil((n - 2) / 2) + 1."""
    return -(-(n - 2) // 2) + 1


def chain(H, W):
    """Map sizes at the five trunk stages: [(H, W), after pool1, .., after pool4]."""
    out = [(H, W)]
    for _ in range(4):
        H, W = pool_out(H), pool_out(W)
        out.append((H, W))
    return out


def trunk_shapes(H, W):
    """[(layer, H, W, Cin, Cout)] of the 13 trunk convolutions for a net input of HxW."""
    ch = chain(H, W)
    out, cin = [], 3
    for name, st in zip(TRUNK_LAYERS, TRUNK_STAGE):
        out.append((name, ch[st][0], ch[st][1], cin, TRUNK_CHANNELS[st]))
        cin = TRUNK_CHANNELS[st]
    return out


def feature_map(h, w):
    H, W, _ = net_input(h, w)
    return chain(H, W)[4]


def anchors(h, w):
    fh, fw = feature_map(h, w)
    return fh * fw * NUM_ANCHORS


# Net inputs whose full-resolution layers (conv1_x, conv2_x: seven eighths of the op-level test's run time, all of it the fp64
# reference on the CPU) are left to their transposed partner in the list: 800x600 <- 600x800, 1000x562 <- 562x1000, 901x600 <-
# 600x901, and 600x600, whose stage 1-2 maps have the row count of 600x800 and the column count of 800x600's partner.  The partial
# tile rows and columns those layers meet stay covered (H = 562, 281, 150, 75, 60, 30; W = 901, 451).  Stages 3-5 keep every shape.
OP_LEVEL_SKIP_STAGE12 = ((800, 600), (1000, 562), (901, 600), (600, 600))


def sweep_conv_cases():
    """The distinct (layer kind, H, W, Cin, Cout) the sweep launches, de-duplicated over the list, in first-use order.  Layer kind:
    "c3" (conv1_1: NCHW input, 3 channels), "pool" (the convolution whose Pooling is fused into its epilogue) or "plain"."""
    seen, out = set(), []
    for h, w, _ in SIZES:
        H, W, _s = net_input(h, w)
        for name, lh, lw, cin, cout in trunk_shapes(H, W):
            if (H, W) in OP_LEVEL_SKIP_STAGE12 and name[:5] in ("conv1", "conv2"):
                continue
            kind = "c3" if name == "conv1_1" else "pool" if name in POOL_AFTER else "plain"
            key = (kind, lh, lw, cin, cout)
            if key not in seen:
                seen.add(key)
                out.append((name,) + key)
    return out


def split_cases():
    """The cases of sweep_conv_cases() the default (throughput) plan runs as transform passes around one batched InnerProduct
    launch (csrc/conv_wino4_split.hip): 512 channels in and out on a map of at least 304 4x4 tiles -- stated here from the shapes
    alone; tests/test_gpu_size_sweep.py holds the library's own rule (mnc_conv3x3_wino4_split_selected) to this list."""
    return [c for c in sweep_conv_cases() if c[4] >= 512 and c[5] >= 512 and -(-c[2] // 4) * -(-c[3] // 4) >= 304]
