"""A plain-Python restatement of the reference's metric sample aggregator, the yardstick of ccmi_aggregator.

Written from cruise-control-core: monitor/sampling/aggregator/{MetricSampleAggregator, RawMetricValues, WindowState,
MetricSampleAggregatorState.computeCompleteness, MetricSampleCompleteness, AggregationOptions, Extrapolation}.java and
common/WindowIndexedArrays.java, method by method and in the reference's statement order. It is not derived from the
HIP code. A Java float is a Python float that numpy.float32 has rounded (f32 below): the sum, quotient or conversion of
floats computed in double and rounded once to float32 is the correctly rounded float32 result (53 >= 2 * 24 + 2), so
f32(a + b) is Java's float a + b. A Java double is a Python float. The reference's completeness and window-state caches
are left out: every query computes from the current bits, which is the reference's answer whenever its caches are
current.
"""
import math

import numpy as np

AVG, MAX, LATEST = 0, 1, 2
NONE, AVG_AVAILABLE, AVG_ADJACENT, FORCED_INSUFFICIENT, NO_VALID_EXTRAPOLATION = range(5)
ENTITY, ENTITY_GROUP = 0, 1
INVALID_INDEX = -1
LONG_MAX = (1 << 63) - 1
FAIL_NONE, FAIL_NO_WINDOW_IN_RANGE, FAIL_NOT_ENOUGH_VALID_WINDOWS = 0, 1, 2
_NAN32 = float(np.float32(np.nan))


def f32(x):
    """(float) x"""
    return float(np.float32(x))


def fdiv32(a, b):
    """Java's float a / float b (b may be 0)."""
    if b == 0:
        return _NAN32 if (a == 0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return f32(a / b)


def jdiv(a, b):
    """Java's long a / long b: truncation toward zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def java_max(a, b):
    if a != a:
        return a
    if b != b:
        return b
    if a == 0.0 and b == 0.0:
        return b if math.copysign(1.0, a) < 0 else a
    return a if a > b else b


def float_bits(values):
    """The bit patterns of float32 values, every NaN as Java's canonical one (Float.floatToIntBits)."""
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits


class NotEnoughValidWindowsException(Exception):
    def __init__(self, msg, failure):
        super().__init__(msg)
        self.failure = failure


class IllegalStateException(Exception):
    pass


class RawMetricValues:
    """RawMetricValues extends WindowIndexedArrays."""

    def __init__(self, num_windows_to_keep, min_samples_per_window, functions):
        if num_windows_to_keep <= 1:
            raise ValueError("The number of windows should be at least 2")
        self.fn = list(functions)
        self.counts = [0] * num_windows_to_keep
        self.values = [[0.0] * num_windows_to_keep for _ in self.fn]  # by metric id, then array index
        self.extrapolations = [False] * num_windows_to_keep
        self.validity = [False] * num_windows_to_keep
        self.min_samples = min_samples_per_window
        self.half_min = max(1, min_samples_per_window // 2)
        self.oldest = LONG_MAX

    # ---- WindowIndexedArrays
    def length(self):
        return len(self.counts)

    def array_index(self, window_index):
        return int(math.fmod(window_index, self.length())) if window_index < 0 else window_index % self.length()

    def current_window_index(self):
        return self.oldest + self.length() - 1

    def last_window_index(self):
        return self.current_window_index() - 1

    def first_array_index(self):
        return self.array_index(self.oldest)

    def last_array_index(self):
        return self.array_index(self.last_window_index())

    def prev_array_index(self, a):
        return INVALID_INDEX if a == self.first_array_index() else (a + self.length() - 1) % self.length()

    def next_array_index(self, a):
        return INVALID_INDEX if a == self.last_array_index() else (a + 1) % self.length()

    def in_valid_window_range(self, w):
        return self.oldest <= w <= self.last_window_index()

    # ---- the bits
    def _reset(self, a):
        self.validity[a] = False
        self.extrapolations[a] = False

    def _update_enough_samples(self, a):
        if self.counts[a] == self.min_samples:
            self.validity[a] = True
            self.extrapolations[a] = False
            return True
        return self.counts[a] >= self.min_samples

    def _update_avg_adjacent(self, a):
        p, n = self.prev_array_index(a), self.next_array_index(a)
        if p == INVALID_INDEX or n == INVALID_INDEX:
            return False
        if self.counts[p] >= self.min_samples and self.counts[n] >= self.min_samples:
            self.validity[a] = True
            self.extrapolations[a] = True
            return True
        return False

    def _update_forced_insufficient(self, a):
        if self.counts[a] > 0:
            self.validity[a] = True
            self.extrapolations[a] = True
            return True
        return False

    def _maybe_update_for(self, a):
        if (not self._update_enough_samples(a) and not self.extrapolations[a]
                and not self._update_forced_insufficient(a) and not self._update_avg_adjacent(a)):
            self._reset(a)

    def _has_two_left(self, a):
        p = self.prev_array_index(a)
        return p != INVALID_INDEX and self.prev_array_index(p) != INVALID_INDEX

    def _has_two_right(self, a):
        n = self.next_array_index(a)
        return n != INVALID_INDEX and self.next_array_index(n) != INVALID_INDEX

    def _maybe_update_prev_and_next_for(self, a):
        if self.counts[a] >= self.min_samples:
            if a != self.array_index(self.current_window_index()) and self._has_two_left(a):
                p = self.prev_array_index(a)
                if self.counts[p] == 0:
                    self._update_avg_adjacent(p)
            if self._has_two_right(a):
                n = self.next_array_index(a)
                if self.counts[n] == 0:
                    self._update_avg_adjacent(n)

    # ---- the calls
    def add_sample(self, sample, window_index):
        if window_index < self.oldest:
            return
        if window_index > self.current_window_index():
            raise ValueError("Cannot add sample to window index %d" % window_index)
        a = self.array_index(window_index)
        c = self.counts[a]
        for m, fn in enumerate(self.fn):
            nv = float(sample[m])
            row = self.values[m]
            if fn == AVG:
                row[a] = f32(nv if c == 0 else row[a] + nv)
            elif fn == MAX:
                row[a] = f32(nv if c == 0 else java_max(row[a], nv))
            else:
                row[a] = f32(nv)
        self.counts[a] = c + 1
        self._maybe_update_for(a)
        self._maybe_update_prev_and_next_for(a)

    def update_oldest_window_index(self, new_oldest):
        prev_last = self.last_window_index()
        if prev_last > LONG_MAX:  # Java's long wraps around on a new instance
            prev_last -= 1 << 64
        self.oldest = new_oldest
        if prev_last >= self.oldest:
            self._maybe_update_for(self.array_index(prev_last))

    def reset_window_indices(self, start, n):
        abandoned = 0
        for i in range(start, start + n):
            a = self.array_index(i)
            abandoned += self.counts[a]
            self.counts[a] = 0
            self._reset(a)
        return abandoned

    def is_valid(self, max_allowed_windows_with_extrapolation):
        cur = self.array_index(self.current_window_index())
        all_valid = sum(self.validity) - (1 if self.validity[cur] else 0) == self.length() - 1
        return all_valid and self.num_windows_with_extrapolation() <= max_allowed_windows_with_extrapolation

    def num_windows_with_extrapolation(self):
        cur = self.array_index(self.current_window_index())
        return sum(self.extrapolations) - (1 if self.extrapolations[cur] else 0)

    def is_valid_at_window_index(self, w):
        return self.validity[self.array_index(w)]

    def is_extrapolated_at_window_index(self, w):
        return self.extrapolations[self.array_index(w)]

    def num_samples(self):
        return sum(self.counts)

    def _get_value(self, m, a):
        if self.counts[a] == 0:
            return 0.0
        if self.fn[m] == AVG:
            return fdiv32(self.values[m][a], float(self.counts[a]))
        return self.values[m][a]

    def aggregate(self, window_indices, check_window=True):
        """-> (values[m][i] as Python floats holding float32 values, extrapolation code per i), in the given order."""
        out = [[0.0] * len(window_indices) for _ in self.fn]
        extrapolations = [NONE] * len(window_indices)
        for m in range(len(self.fn)):
            vals = self.values[m]
            for i, w in enumerate(window_indices):
                if check_window and not self.in_valid_window_range(w):
                    raise ValueError("Index %d is out of range" % w)
                a = self.array_index(w)
                c = self.counts[a]
                if c >= self.half_min:
                    out[m][i] = self._get_value(m, a)
                    if c < self.min_samples:
                        extrapolations[i] = AVG_AVAILABLE
                elif (a != self.first_array_index() and a != self.last_array_index()
                      and self.counts[self.prev_array_index(a)] >= self.min_samples
                      and self.counts[self.next_array_index(a)] >= self.min_samples):
                    extrapolations[i] = AVG_ADJACENT
                    p, n = self.prev_array_index(a), self.next_array_index(a)
                    total = f32(f32(vals[p] + (0.0 if c == 0 else vals[a])) + vals[n])  # a float sum, then widened
                    if self.fn[m] == AVG:
                        out[m][i] = f32(total / (self.counts[p] + c + self.counts[n]))
                    else:
                        out[m][i] = f32(total / (3 if c > 0 else 2))
                elif c > 0:
                    out[m][i] = self._get_value(m, a)
                    extrapolations[i] = FORCED_INSUFFICIENT
                else:
                    out[m][i] = 0.0
                    extrapolations[i] = NO_VALID_EXTRAPOLATION
        return out, extrapolations


class AggregationOptions:
    def __init__(self, min_valid_entity_ratio, min_valid_entity_group_ratio, min_valid_windows,
                 max_allowed_extrapolations_per_entity, granularity=ENTITY, include_invalid_entities=False):
        if min_valid_windows < 1:
            raise ValueError("The minimum valid windows must be at least 1")
        self.min_valid_entity_ratio = float(min_valid_entity_ratio)
        self.min_valid_entity_group_ratio = float(min_valid_entity_group_ratio)
        self.min_valid_windows = min_valid_windows
        self.max_allowed_extrapolations_per_entity = max_allowed_extrapolations_per_entity
        self.granularity = granularity
        self.include_invalid_entities = include_invalid_entities


class MetricSampleCompleteness:
    def __init__(self, generation):
        self.generation = generation
        self.windows = []  # every window walked, newest first
        self.included = []  # per walked window
        self.valid_entity_ratio_by_window = []
        self.valid_entity_ratio_with_group_granularity_by_window = []
        self.valid_entity_group_ratio_by_window = []
        self.extrapolated_entities_by_window = []
        self.valid_window_indices = []  # newest first
        self.valid_entities = set()
        self.valid_entity_groups = set()
        self.valid_entity_ratio = 0.0
        self.valid_entity_group_ratio = 0.0
        self.num_interested_entities = 0
        self.num_interested_groups = 0
        self.failure = FAIL_NONE


class AggregationResult:
    def __init__(self, completeness, entities, values, extrapolations, invalid):
        self.completeness = completeness
        self.entities = entities  # ascending ids
        self.values = values  # float32 [k][M][Wv], valid windows newest first
        self.extrapolations = extrapolations  # uint8 [k][Wv]
        self.invalid = invalid  # uint8 [k]


class MetricSampleAggregator:
    def __init__(self, num_windows, window_ms, min_samples_per_window, functions, entity_group):
        self.num_windows = num_windows
        self.window_ms = window_ms
        self.num_windows_to_keep = num_windows + 1
        self.min_samples = min_samples_per_window
        self.fn = list(functions)
        self.group = list(entity_group)
        self.raw = {}  # _rawMetrics
        self.generation = 0
        self.current = 0
        self.oldest = 0

    def window_index(self, time_ms):
        return jdiv(time_ms, self.window_ms) + 1

    def add_sample(self, entity, time_ms, values):
        w = self.window_index(time_ms)
        if w < self.oldest:
            return False
        rolled = self._maybe_roll_out_new_window(w)
        raw = self.raw.get(entity)
        if raw is None:
            raw = RawMetricValues(self.num_windows_to_keep, self.min_samples, self.fn)
            raw.update_oldest_window_index(self.oldest)
            self.raw[entity] = raw
        raw.add_sample(values, w)
        if rolled or w != self.current:
            self.generation += 1
        return True

    def add_samples(self, entities, times, values):
        return [self.add_sample(int(e), int(t), v) for e, t, v in zip(entities, times, values)]

    def _maybe_roll_out_new_window(self, w):
        if self.current < w:
            prev_oldest = self.oldest
            self.oldest = max(1, w - self.num_windows)
            n_reset = min(self.num_windows_to_keep, self.oldest - prev_oldest)
            if n_reset > 0:
                for raw in self.raw.values():
                    raw.update_oldest_window_index(self.oldest)
                    raw.reset_window_indices(prev_oldest, n_reset)
            self.current = w
            return True
        return False

    # ---- the small queries
    def num_available_windows(self, frm=-1, to=LONG_MAX):
        from_w = max(self.window_index(frm), self.oldest)
        to_w = min(self.window_index(to), self.current - 1)
        return max(0, to_w - from_w + 1)

    def all_windows(self):
        return [] if not self.raw else [i * self.window_ms for i in range(self.oldest, self.current + 1)]

    def available_windows(self):
        return [] if not self.raw else [i * self.window_ms for i in range(self.oldest, self.current)]

    def earliest_window(self):
        return None if not self.raw else self.oldest * self.window_ms

    def num_samples(self):
        return sum(r.num_samples() for r in self.raw.values())

    def remove_entities(self, entities):
        removed = False
        for e in set(int(x) for x in entities):
            if e in self.raw:
                del self.raw[e]
                removed = True
        if removed:
            self.generation += 1

    def clear(self):
        self.raw.clear()
        self.generation += 1

    # ---- completeness
    def _interpret(self, interested):
        """interpretAggregationOptions: an empty interested set means every entity with raw metrics."""
        ids = set(int(e) for e in interested) if interested is not None else set()
        return sorted(self.raw.keys()) if not ids else sorted(ids)

    def completeness(self, frm, to, options, interested=None):
        from_w = max(self.window_index(frm), self.oldest)
        to_w = min(self.window_index(to), self.current - 1)
        if from_w > self.current or to_w < self.oldest:
            return MetricSampleCompleteness(self.generation)
        return self._compute_completeness(from_w, to_w, options, self._interpret(interested))

    def _compute_completeness(self, from_w, to_w, opt, entities):
        c = MetricSampleCompleteness(self.generation)
        groups = set(self.group[e] for e in entities)
        c.num_interested_entities, c.num_interested_groups = len(entities), len(groups)
        c.valid_entities = set(entities)
        c.valid_entity_groups = set(groups)
        included_extrapolations = {}
        total_e, total_g = float(len(entities)), float(len(groups))
        for w in range(self.current - 1, self.oldest - 1, -1):  # _windowStates, newest first
            if w > to_w:
                continue
            if w < from_w:
                break
            # getWindowState
            valid_set, extrapolated_set = set(), set()
            for e, raw in self.raw.items():
                if raw.is_extrapolated_at_window_index(w):
                    extrapolated_set.add(e)
                if raw.is_valid_at_window_index(w):
                    valid_set.add(e)
            # WindowState.maybeInclude: fillInValidRatios
            num_extrapolated = 0
            valid_by_group = {}
            invalid_groups = set()
            valid_for_window = set()
            for e in entities:
                g = self.group[e]
                if e in valid_set:
                    addition = 0
                    if e in extrapolated_set:
                        num_extrapolated += 1
                        addition = 1
                    if included_extrapolations.get(e, 0) + addition <= opt.max_allowed_extrapolations_per_entity:
                        valid_for_window.add(e)
                        valid_by_group[g] = valid_by_group.get(g, 0) + 1
                    else:
                        invalid_groups.add(g)
                else:
                    invalid_groups.add(g)
            with_group_granularity = len(valid_for_window)
            for g in invalid_groups:
                count = valid_by_group.pop(g, None)
                if count is not None:
                    with_group_granularity -= count
            valid_groups_for_window = set(valid_by_group.keys())
            c.windows.append(w)
            c.valid_entity_ratio_by_window.append(fdiv32(float(len(valid_for_window)), total_e))
            c.valid_entity_ratio_with_group_granularity_by_window.append(fdiv32(float(with_group_granularity), total_e))
            c.extrapolated_entities_by_window.append(fdiv32(float(num_extrapolated), total_e))
            c.valid_entity_group_ratio_by_window.append(fdiv32(float(len(valid_by_group)), total_g))
            if opt.granularity == ENTITY_GROUP:
                valid_for_window = set(e for e in valid_for_window if self.group[e] in valid_groups_for_window)
            n_e = len(c.valid_entities & valid_for_window)
            n_g = len(c.valid_entity_groups & valid_groups_for_window)
            include = (n_e > 0 and fdiv32(float(n_e), total_e) >= opt.min_valid_entity_ratio
                       and n_g > 0 and fdiv32(float(n_g), total_g) >= opt.min_valid_entity_group_ratio)
            c.included.append(include)
            if include:
                c.valid_entities &= valid_for_window
                c.valid_entity_groups &= valid_groups_for_window
                c.valid_window_indices.append(w)
                for e in valid_for_window:
                    if e in extrapolated_set:
                        included_extrapolations[e] = included_extrapolations.get(e, 0) + 1
        if not c.valid_window_indices:
            c.valid_entities = set()
            c.valid_entity_groups = set()
        c.valid_entity_ratio = fdiv32(float(len(c.valid_entities)), total_e)
        c.valid_entity_group_ratio = fdiv32(float(len(c.valid_entity_groups)), total_g)
        return c

    # ---- aggregate
    def aggregate(self, frm, to, options, interested=None):
        from_w = max(self.window_index(frm), self.oldest)
        to_w = min(self.window_index(to), self.current - 1)
        if from_w > self.current or to_w < self.oldest:
            raise NotEnoughValidWindowsException("There is no window available in range [%d, %d]" % (frm, to),
                                                 FAIL_NO_WINDOW_IN_RANGE)
        entities = self._interpret(interested)
        c = self._compute_completeness(from_w, to_w, options, entities)
        # validateCompleteness
        if len(c.valid_window_indices) < options.min_valid_windows:
            raise NotEnoughValidWindowsException("There are only %d valid windows" % len(c.valid_window_indices),
                                                 FAIL_NOT_ENOUGH_VALID_WINDOWS)
        if c.valid_entity_ratio < options.min_valid_entity_ratio:
            raise IllegalStateException("The entity coverage %.3f in range [%d, %d]" % (c.valid_entity_ratio, frm, to))
        if c.valid_entity_group_ratio < options.min_valid_entity_group_ratio:
            raise IllegalStateException("The entity group coverage %.3f in range [%d, %d]"
                                        % (c.valid_entity_group_ratio, frm, to))
        windows = c.valid_window_indices
        covered = entities if options.include_invalid_entities else sorted(c.valid_entities)
        k, m_n, w_n = len(covered), len(self.fn), len(windows)
        empty = ([[0.0] * w_n for _ in range(m_n)], [NO_VALID_EXTRAPOLATION] * w_n)  # ValuesAndExtrapolations.empty
        rows, codes, invalid = [], [], []
        for e in covered:
            raw = self.raw.get(e)
            vals, ext = empty if raw is None else raw.aggregate(windows)
            rows.append(vals)
            codes.append(ext)
            invalid.append(1 if raw is None or not raw.is_valid(options.max_allowed_extrapolations_per_entity) else 0)
        values = np.array(rows, dtype=np.float64).astype(np.float32).reshape(k, m_n, w_n)  # exact: float32 values
        return AggregationResult(c, np.array(covered, dtype=np.int32), values,
                                 np.array(codes, dtype=np.uint8).reshape(k, w_n), np.array(invalid, dtype=np.uint8))

    def peek_current_window(self):
        """-> (entities ascending, values float32 [k][M], extrapolation code [k]) for every entity with raw metrics."""
        ents = sorted(self.raw.keys())
        rows, codes = [], []
        for e in ents:
            vals, x = self.raw[e].aggregate([self.current], check_window=False)
            rows.append([v[0] for v in vals])
            codes.append(x[0])
        values = np.array(rows, dtype=np.float64).astype(np.float32).reshape(len(ents), len(self.fn))
        return np.array(ents, dtype=np.int32), values, np.array(codes, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ seeded scripts
GROUP_SIZES = (1, 2, 63, 64, 65, 100, 5)  # 300 entities; a wave is 64 lanes
SCRIPT_WINDOWS = (1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 18, 19, 20, 21)  # a leap of 8 windows, 21 > 12: the buffer wraps twice
SPARSE_WINDOW = 4  # a handful of samples only: two roll-outs fall into one batch, and its ratios exclude it
NEVER_SAMPLED = 123
REMOVED = (5, 17, 100, 250)
WINDOW_MS = 1000


def interleaved_groups(rng, sizes=GROUP_SIZES):
    group = [g for g, n in enumerate(sizes) for _ in range(n)]
    rng.shuffle(group)
    return group


def random_script(seed, num_metrics):
    """-> (entity_group, steps). A step is ("add", entities, times_ms, values[n][M]), ("remove", ids) or ("query",).
    Samples come window by window in SCRIPT_WINDOWS order; within a window an entity gets 4..6 samples (mostly), 2..3,
    1 or none, a few samples are stamped into older windows and a few too old to be kept; the stream is cut into
    batches of up to 500 wherever it falls, so roll-outs happen inside batches."""
    import random

    rng = random.Random(seed)
    group = interleaved_groups(rng)
    num_entities = len(group)
    stream = []
    marks = {}  # stream position -> steps to insert before the batch that starts at or after it
    for wi, w in enumerate(SCRIPT_WINDOWS):
        samples = []
        for e in range(num_entities):
            if e == NEVER_SAMPLED:
                continue
            roll = rng.random()
            if w == SPARSE_WINDOW:
                count = 1 if roll < 0.03 else 0
            else:
                count = rng.randrange(4, 7) if roll < 0.70 else rng.randrange(2, 4) if roll < 0.80 else \
                    1 if roll < 0.88 else 0
            for _ in range(count):
                target = w
                roll = rng.random()
                if roll < 0.05:
                    target = max(1, w - rng.randrange(1, 4))  # an old window that is still kept
                elif roll < 0.07:
                    target = max(1, w - 8)  # too old once the oldest window has moved on
                t = (target - 1) * WINDOW_MS + rng.randrange(0, WINDOW_MS)
                vals = [rng.choice([rng.uniform(0.0, 1e5), float(rng.randrange(0, 1000)), rng.random()])
                        for _ in range(num_metrics)]
                samples.append((e, t, vals))
        rng.shuffle(samples)
        if wi in (3, 8, 11, 13):
            marks[len(stream)] = [("query",)]
        if wi == 9:
            marks[len(stream)] = [("remove", list(REMOVED)), ("query",)]
        stream += samples
    steps = []
    pos = 0
    pending = sorted(marks)
    while pos < len(stream):
        while pending and pending[0] <= pos:
            steps += marks[pending.pop(0)]
        n = rng.randrange(200, 501)
        chunk = stream[pos:pos + n]
        pos += n
        steps.append(("add", [s[0] for s in chunk], [s[1] for s in chunk], [s[2] for s in chunk]))
    steps.append(("query",))
    return group, steps


def query_matrix(num_entities, rng):
    """The (options, interested mask or None) of one query point."""
    out = []
    mask = [1 if rng.random() < 0.6 else 0 for _ in range(num_entities)]
    mask[NEVER_SAMPLED] = 1
    for granularity in (ENTITY, ENTITY_GROUP):
        for max_extrapolations in (0, 1, 5):
            for ratios in ((0.0, 0.0), (0.5, 0.3)):
                for interested in (None, mask):
                    for include_invalid in (False, True):
                        out.append((AggregationOptions(ratios[0], ratios[1], 1, max_extrapolations, granularity,
                                                       include_invalid), interested))
    return out
