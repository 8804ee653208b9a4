"""Python mirror of cpp/o3s_submap_collection.hpp (the host bookkeeping of o3d_slam::SubmapCollection,
open3d_slam/src/SubmapCollection.cpp:94-247, over device-resident submaps): used by the tests to check the compiled header
step by step and by tools/mapping_loop.py.  No compute here — every cloud operation is a call into the C-ABI library."""
import numpy as np

from . import cloud_ops as co
from .mapper import mul4
from .submap import AssembledMap, ProcessedScan, Submap, transform_submaps


INT_MAX = 2**31 - 1   # std::numeric_limits<int>::max()
VOXEL_EXPANSION_FACTOR_ADJACENCY_BASED_REVISITING = 2.5   # magic.hpp:16


class SubmapCollection:
    """SubmapCollection::insertScan / updateActiveSubmap (SubmapCollection.cpp:94-247) restated over the Python mirror — the
    same steps as cpp/o3s_submap_collection.hpp, resident scans in a ring of numScansOverlap + 1 objects."""

    def __init__(self, radius, min_num, max_points, overlap, map_voxel, map_builder_cropper, submap_factory=None, scan_factory=None,
                 transform_maps=None, assemble_maps=None, odometry_constraints_call=None, refine_call=None):
        """map_builder_cropper: (kind, p0[, p1, p2]) as for cloud_ops.croppingVolumeFactory.  submap_factory / scan_factory:
        stand-ins for the device-resident objects (insertProcessed / __len__ / computeSubmapCenter) — the CPU tests of the
        switching rules use them; the default is the real thing.  transform_maps(maps, Ts): the one batched device call of
        transform() (submap.transform_submaps unless a stand-in is given).  assemble_maps(out, maps, voxel_size, normals, colors):
        the one device call of assembleMap() (AssembledMap.build unless a stand-in is given).  odometry_constraints_call / refine_call:
        the device calls of the odometry constraints (constraint_builders.submaps_odometry_constraints and the refinement unless
        stand-ins are given)."""
        self._odometry_call, self._refine_call = odometry_constraints_call, refine_call
        self.refine_odometry_constraints = False   # isRefineOdometryConstraintsBetweenSubmaps_ (Parameters.hpp:177; every parameter file: false)
        self.odometry_constraints = []             # SubmapCollection::odometryConstraints_
        self.loop_closure_candidates = []          # loopClosureCandidatesIdxs_: (submap id, time stamp)
        self._transform_maps = transform_maps or transform_submaps
        self._assemble_maps = assemble_maps or AssembledMap.build
        self.radius, self.min_num, self.max_points, self.overlap = radius, min_num, max_points, overlap
        self.map_voxel, self.cropper = map_voxel, tuple(map_builder_cropper)
        self._new_submap = submap_factory or (lambda: Submap(self.map_voxel, co.croppingVolumeFactory(*self.cropper)))
        scan_factory = scan_factory or ProcessedScan
        self.maps, self.ids, self.parents, self.origins, self.centers = [], [], [], [], []
        self.range_sensor_poses = []   # Submap::mapToRangeSensor_ of every submap: the pose of the last scan that went into it
        self.dense_maps = {}           # submap index -> dense map object (transform(T)), where the driver keeps one
        self.active, self.next_id, self.merged, self.force = 0, 0, 0, False
        self.edges = set()
        self.loop_closure_flags = {}   # AdjacencyMatrix::isLoopClosureSubmap_: submap id -> flag, an entry per id an edge has named
        self.buffer, self.free = [], [scan_factory() for _ in range(overlap + 1)]
        self.finished, self.finished_queue, self.switched = [], [], False
        # SubmapParams of cpp/o3s_submap_collection.hpp: adjacency_based_revisiting_min_fitness, and whether the revisit check of
        # SubmapCollection.cpp:392-407 runs at all (off = the reference as it runs: its body is commented out and returns true)
        self.adjacency_min_fitness = 0.4
        self.check_switching_consistency = False
        self.last_switch_fitness = float("nan")   # fitness of the last consistency check (NaN: the last insert made none)
        self.create(np.zeros(3))

    def create(self, origin):
        self.maps.append(self._new_submap())
        self.ids.append(self.next_id)
        self.parents.append(self.active)
        self.next_id += 1
        self.origins.append(np.array(origin, np.float64))
        self.centers.append(None)
        self.range_sensor_poses.append(np.eye(4))
        self.active = len(self.maps) - 1
        self.merged = 0

    def centre(self, i):
        return self.centers[i] if self.centers[i] is not None else self.origins[i]

    @staticmethod
    def dist(a, b):
        d = a - b
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])

    def scan_for_next(self):
        return self.free[-1]

    def adjacent(self, a, b):
        return a == b or (min(a, b), max(a, b)) in self.edges

    def add_edge(self, a, b):
        """AdjacencyMatrix::addEdge (AdjacencyMatrix.cpp:16-21): the edge, and BOTH ends lose their loop-closure flag."""
        self.edges.add((min(a, b), max(a, b)))
        self.loop_closure_flags[a] = False
        self.loop_closure_flags[b] = False

    def markAsLoopClosureSubmap(self, i):
        """AdjacencyMatrix::markAsLoopClosureSubmap (:57-59): `.at(id)` — KeyError for an id no edge has named."""
        if i not in self.loop_closure_flags:
            raise KeyError(i)
        self.loop_closure_flags[i] = True

    def getDistanceToNearestLoopClosureSubmap(self, i) -> int:
        """AdjacencyMatrix::getDistanceToNearestLoopClosureSubmap (:23-55) as written: INT_MAX while no edge has been added; else a
        breadth-first walk from `i` (neighbours in ascending id, std::set's order) that stops at the first flagged submap it takes
        from the queue — or, when none is reachable, at the LAST submap it visits — and returns max(0, hops to it - 1)."""
        if not self.loop_closure_flags:
            return INT_MAX
        neighbours = {}
        for a, b in self.edges:
            if a != b:
                neighbours.setdefault(a, set()).add(b)
                neighbours.setdefault(b, set()).add(a)
        queue, visited, parents = [i], {i}, {}
        v = i
        while queue:
            v = queue.pop(0)
            if self.loop_closure_flags.get(v, False):   # (an id only a directly added edge names carries no flag)
                break
            for adj in sorted(neighbours.get(v, ())):
                if adj not in visited:
                    visited.add(adj)
                    queue.append(adj)
                    parents[adj] = v
        distance = 0
        while v != i:
            v = parents[v]
            distance += 1
        return max(0, distance - 1)

    def computeFeatures(self, i, params=None, keypoints=None):
        """Submap::computeFeatures of submap i (Submap.cpp:255-275): the feature set and, with it, the occupancy snapshot voxelMap_ at
        2.5 x the map voxel size (:239-240, :260-264).  Returns the number of sparse points.
        With a list of finished (submap id, time stamp) instead of an index: SubmapCollection::computeFeatures(finishedSubmapIds)
        (SubmapCollection.cpp:257-281) — the features of every finished submap, each pushed to the loop-closure candidates, and the
        odometry constraints of the finished submaps into the collection's own list (one device call).  The reference runs the
        features on a second thread; here the two steps run one after the other on the caller (both settle and use the streams of
        the same submaps).  Returns the list of sparse-point counts.
        keypoints (cloud_ops.iss_params; None = off): ISS keypoint selection right behind the features of each submap
        (Submap.selectKeypoints) — the feature set that place recognition searches is then the keypoints' alone, and the count
        returned is theirs."""
        if not isinstance(i, (int, np.integer)):
            from .constraint_builders import compute_odometry_constraints

            finished = [(int(f[0]), f[1]) for f in i]
            counts = []
            for f in finished:
                counts.append(self.computeFeatures(f[0], params, keypoints))
                self.loop_closure_candidates.append(f)
            compute_odometry_constraints(self, self.odometry_constraints, finished, self._odometry_call, self._refine_call)
            return counts
        n = self.maps[i].computeFeatures(params)
        if keypoints is not None:
            n = len(self.maps[i].selectKeypoints(keypoints)[0])
        if self.map_voxel > 0.0:
            self.maps[i].buildVoxelMap(VOXEL_EXPANSION_FACTOR_ADJACENCY_BASED_REVISITING * self.map_voxel)
        return n

    def isSwitchingSubmapsConsistant(self, ps, candidate, T) -> bool:
        """SubmapCollection::isSwitchingSubmapsConsistant (:392-407) as written in its commented body, over the resident merge cloud
        of `ps`.  A candidate without a snapshot has fitness 0, an empty scan NaN: both False."""
        _, self.last_switch_fitness = self.maps[candidate].overlapFitness(ps, T, 0)
        return self.last_switch_fitness > self.adjacency_min_fitness

    def update_active(self, p0, ps=None, T=None):
        if self.force:
            self.create(p0)
            self.force = False
            return
        if self.merged < self.min_num:
            return
        closest = 0
        for i in range(1, len(self.maps)):
            if self.dist(p0, self.centre(i)) < self.dist(p0, self.centre(closest)):
                closest = i
        active = self.active
        if len(self.maps[active]) > self.max_points:
            self.force = True
        if self.dist(p0, self.centre(closest)) < self.radius:
            if closest == active:
                return
            if self.adjacent(self.ids[closest], self.ids[active]) and \
                    (not self.check_switching_consistency or self.isSwitchingSubmapsConsistant(ps, closest, T)):
                self.active = closest
            elif self.dist(p0, self.centre(active)) > self.radius:
                self.create(p0)
        else:
            self.create(p0)

    def insert(self, ps, T, stamp):
        self.switched = False
        prev = self.active
        assert self.free and self.free[-1] is ps
        self.free.pop()
        self.buffer.append((ps, T.copy(), stamp))
        while len(self.buffer) > self.overlap:
            self.free.append(self.buffer.pop(0)[0])
        self.last_switch_fitness = float("nan")
        self.update_active(T[:3, 3].copy(), ps, T)
        if prev != self.active:
            self.switched = True
            self._insert_into(prev, ps, T)
            self.centers[prev] = self.maps[prev].computeSubmapCenter()
            self.finished.append((prev, stamp))
            self.finished_queue.append((prev, stamp))
            self.merged = 0
            self.add_edge(self.ids[prev], self.ids[self.active])
            while self.buffer:
                q, Tq, _ = self.buffer.pop(0)
                self._insert_into(self.active, q, Tq)
                self.free.append(q)
            assert len(self.maps[self.active]) > 0
        else:
            self._insert_into(self.active, ps, T)
        self.merged += 1

    def _insert_into(self, i, ps, T):
        self.range_sensor_poses[i] = np.array(T, np.float64)   # Submap.cpp:45
        self.maps[i].insertProcessed(ps, T)

    def getOdometryConstraints(self):
        """SubmapCollection::getOdometryConstraints (:287-289)"""
        return self.odometry_constraints

    def popLoopClosureCandidates(self):
        """loopClosureCandidatesIdxs_.popAllElements(), as SlamWrapper's workers take them"""
        out, self.loop_closure_candidates = self.loop_closure_candidates, []
        return out

    def pop_finished(self):
        """SubmapCollection::popFinishedSubmapIds (:53-55)."""
        out, self.finished_queue = self.finished_queue, []
        return out

    def update_adjacency_matrix(self, loop_closure_constraints):
        """SubmapCollection::updateAdjacencyMatrix (:75-81): a loop-closure constraint makes its two submaps adjacent and marks
        both as loop-closure submaps."""
        for c in loop_closure_constraints:
            a, b = c.source_submap_idx, c.target_submap_idx
            self.add_edge(a, b)
            self.markAsLoopClosureSubmap(a)
            self.markAsLoopClosureSubmap(b)

    def getTotalNumPoints(self) -> int:
        """SubmapCollection::getTotalNumPoints (:69-73): the sum of the submaps' map sizes."""
        return sum(len(m) for m in self.maps)

    def assembleMap(self, out: AssembledMap, voxel_size=0.0, normals=True, colors=True) -> int:
        """Mapper::getAssembledMapPointCloud's loop over the collection (Mapper.cpp:524-535) as one device call: every submap in
        index order — the active one is not special — into `out`; voxel_size > 0 down-samples the assembled cloud the way
        SlamWrapperRos::publishMaps does.  Returns the size of the result."""
        return self._assemble_maps(out, list(self.maps), voxel_size, normals, colors)

    def transform(self, increments):
        """SubmapCollection::transform (:324-375).  increments: objects with .dT (4x4) and .submap_id.  A submap an increment names
        gets that increment; every other submap walks up its parents until one is not among the unnamed submaps and takes
        increments[parent] — a POSITIONAL lookup, as written (:362).  All device work is one batched call; per submap also
        (Submap.cpp:115-128) mapToRangeSensor_ = mapToRangeSensor_ * T, submapCenter_ = T * submapCenter_ and the dense map, where
        one is kept.  The overlap buffer is flushed: its scan objects go back to the free ring."""
        increments = list(increments)
        n = len(self.maps)
        plan = []                                    # (submap index, T) in the reference's order of application
        optimized = []
        for u in increments:
            if u.submap_id < n:
                plan.append((u.submap_id, np.asarray(u.dT, np.float64)))
                optimized.append(u.submap_id)
            # else: "trying to update submap ... but there are only ..." (:337): reported and skipped by the reference
        to_update = [i for i in range(n) if i not in set(optimized)]
        for idx in to_update:
            current = idx
            while increments:                        # "while (true && !transformIncrements.empty())"
                current = self.parents[current]
                if current not in to_update:         # the parent is in the pose graph
                    plan.append((idx, np.asarray(increments[current].dT, np.float64)))   # .at(currentNode): IndexError out of range
                    break
                if current == self.parents[current]:
                    raise RuntimeError("Stuck in a loop, this should not happen")
        if len({i for i, _ in plan}) != len(plan):
            # (the reference would transform such a submap twice; the batched device call takes every submap once)
            raise ValueError("SubmapCollection.transform: a submap is named by more than one increment")
        if plan:
            self._transform_maps([self.maps[i] for i, _ in plan], [T for _, T in plan])
        for i, T in plan:
            self.range_sensor_poses[i] = mul4(self.range_sensor_poses[i], T)
            if self.centers[i] is not None:          # (submapCenter_ is zero until it is computed; nobody reads it before)
                c = self.centers[i]
                v = [((T[r, 0] * c[0] + T[r, 1] * c[1]) + T[r, 2] * c[2]) + T[r, 3] for r in range(3)]
                self.centers[i] = np.array(v)
            if i in self.dense_maps:
                self.dense_maps[i].transform(T)
        while self.buffer:                           # :374 overlapScansBuffer_.clear()
            self.free.append(self.buffer.pop(0)[0])
