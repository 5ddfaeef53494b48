"""Kinetics-Skeleton (OpenPose 18-joint) graph (reference ``graph/kinetics.py:26-51``)."""
from . import tools

num_node = 18
self_link = [(i, i) for i in range(num_node)]
inward = [(4, 3), (3, 2), (7, 6), (6, 5), (13, 12), (12, 11), (10, 9), (9, 8), (11, 5),
          (8, 2), (5, 1), (2, 1), (0, 1), (15, 0), (14, 0), (17, 15), (16, 14)]
outward = [(j, i) for (i, j) in inward]
neighbor = inward + outward
# parent of every joint for the bone stream (ops.skeleton_streams): the 0-based pairs of the reference's
# data_gen/gen_bone_data.py:24-27.  Stated as data, NOT derived from `inward`: there joint 0 points at joint 1, here
# joint 0 is its own parent and joint 1 points at joint 0.
bone_parents = [0, 0, 1, 2, 3, 1, 5, 6, 2, 8, 9, 5, 11, 12, 0, 0, 14, 15]


class Graph:
    def __init__(self, labeling_mode='spatial'):
        self.num_node = num_node
        self.self_link = self_link
        self.inward = inward
        self.outward = outward
        self.neighbor = neighbor
        self.bone_parents = list(bone_parents)
        self.A = self.get_adjacency_matrix(labeling_mode)

    def get_adjacency_matrix(self, labeling_mode=None):
        if labeling_mode is None:
            return self.A
        if labeling_mode == 'spatial':
            return tools.spatial_graph(num_node, self_link, inward, outward)
        raise ValueError(labeling_mode)
