"""numpy restatement of jueying_slam's localisation map logic, written from the reference lines and not from the library:
is_in_area / create_pcd (include/dynamic_map.h:114-156), the reload trigger of dynamic_load_map_run (localization.cpp:295-300) and
dynamic_load_map's pcl::PassThrough crop (localization.cpp:256-280).

pcl::PassThrough is not in the reference tree; the rule used here: setFilterLimits takes floats, so a limit is
the double expression rounded once to float; a point passes iff lo <= v <= hi in float; a point with any non-finite x, y or z is
dropped and counted whatever the window says."""
import numpy as np

F = np.float32
NEVER = F(-999999.0)


def is_in_area(x, y, box, m):
    """dynamic_map.h:114-117 in double; box = x_min, y_min, z_min, x_max, y_max, z_max."""
    x, y, m = float(x), float(y), float(m)
    return (float(box[0]) - m) <= x and x <= (float(box[3]) + m) and (float(box[1]) - m) <= y and y <= (float(box[4]) + m)


def select(boxes, p_x, p_y, margin):
    """create_pcd(const float& p_x, const float& p_y, areas, path, float margin): indices in list order.  margin < 0: the node loads
    every area once (localization.cpp:229-242)."""
    p_x, p_y, m = F(p_x), F(p_y), F(margin)
    if m < 0:
        return np.arange(len(boxes), dtype=np.int32)
    return np.array([i for i, b in enumerate(boxes) if is_in_area(p_x, p_y, b, m)], np.int32)


def need_load(pose, last_load, area_size):
    """localization.cpp:295-300: float differences, float sum of squares left to right, float sqrt, int area_size as float."""
    dx = F(F(pose[3]) - F(last_load[3]))
    dy = F(F(pose[4]) - F(last_load[4]))
    dz = F(F(pose[5]) - F(last_load[5]))
    with np.errstate(over="ignore"):
        s = F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))
        d = F(np.sqrt(s))
    return bool(d > F(int(area_size)))


def limits(pose_v, max_range):
    """setFilterLimits(pose - max_range * 1.1, pose + max_range * 1.1): float - float * double, then float arguments."""
    lo = float(F(pose_v)) - float(F(max_range)) * 1.1
    hi = float(F(pose_v)) + float(F(max_range)) * 1.1
    return F(lo), F(hi)


def window(pose, max_range, margin):
    """(x_lo, x_hi, y_lo, y_hi); margin < 0: dynamic_load_map does nothing, the whole map is kept (infinite limits)."""
    if int(margin) < 0:
        return F(-np.inf), F(np.inf), F(-np.inf), F(np.inf)
    return limits(pose[3], max_range) + limits(pose[4], max_range)


def concat(tiles, sel):
    """*pcd += *part over the selected areas in list order; an empty tile contributes nothing."""
    parts = [np.asarray(tiles[int(i)], F).reshape(-1, 4) for i in sel]
    return np.concatenate(parts) if parts else np.zeros((0, 4), F)


def crop_cloud(cloud, win, crop_x):
    """(kept, number of non-finite points dropped) of one concatenated cloud, order kept."""
    x_lo, x_hi, y_lo, y_hi = win
    c = np.asarray(cloud, F)
    fin = np.isfinite(c[:, 0]) & np.isfinite(c[:, 1]) & np.isfinite(c[:, 2])
    with np.errstate(invalid="ignore"):
        keep = fin & (y_lo <= c[:, 1]) & (c[:, 1] <= y_hi)
        if crop_x:
            keep = keep & (x_lo <= c[:, 0]) & (c[:, 0] <= x_hi)
    return c[keep], int((~fin).sum())


def crop(lists, sels, pose, max_range=150.0, margin=-1, crop_x=0):
    """dynamic_load_map on the loaded tiles.  lists: ((corner_boxes, corner_tiles), (surf_boxes, surf_tiles)); sels: the two
    selections.  Returns dict(corner, surf, nonfinite, window, corner_in, surf_in)."""
    win = window(pose, max_range, margin)
    cin = concat(lists[0][1], sels[0])
    sin = concat(lists[1][1], sels[1])
    co, nf0 = crop_cloud(cin, win, crop_x)
    su, nf1 = crop_cloud(sin, win, crop_x)
    return {"corner": co, "surf": su, "nonfinite": nf0 + nf1, "window": win, "corner_in": len(cin), "surf_in": len(sin)}
