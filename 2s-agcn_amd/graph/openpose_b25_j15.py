"""OpenPose BODY_25 reduced to its first 15 joints (reference ``graph/openpose_b25_j15.py``): 0 nose, 1 neck,
2-4 right arm, 5-7 left arm, 8 mid hip, 9-11 right leg, 12-14 left leg.  Every bone points towards the neck."""
from . import tools

num_node = 15
self_link = [(i, i) for i in range(num_node)]
_chains = [(0, 1),                    # nose -> neck
           (4, 3, 2, 1),              # right wrist -> elbow -> shoulder -> neck
           (7, 6, 5, 1),              # left arm
           (8, 1),                    # mid hip -> neck
           (11, 10, 9, 8),            # right ankle -> knee -> hip -> mid hip
           (14, 13, 12, 8)]           # left leg
inward = [(a, b) for chain in _chains for a, b in zip(chain[:-1], chain[1:])]
outward = [(j, i) for (i, j) in inward]
neighbor = inward + outward
# parent of every joint for the bone stream (ops.skeleton_streams).  The reference's data_gen/gen_bone_data.py has no
# table for this skeleton, so this one has no reference counterpart: the parents are this graph's own (child, parent)
# edges, and the neck (joint 1), which every bone points towards, is its own parent.
bone_parents = [dict(inward).get(v, v) for v in range(num_node)]


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
