"""A NumPy restatement of ntk_track_decode_mask, written from the rules in include/ntmtrack.h (NTK_CLIPDEC_*), one frame of one
slot at a time: the oracle of tests/test_validate_files_gpu.py."""
import numpy as np

DECODED, FAILED, MASKED, FIRST_FAILED, FIRST_STATUS, START_STATUS, HEAD = 0, 1, 2, 3, 4, 5, 6
BAD_DESC = 4                                            # NTK_JPEG_STATUS_BAD_DESC


def new_table(n_clips):
    table = np.zeros((n_clips, HEAD), dtype=np.int64)
    table[:, FIRST_FAILED] = -1                         # the owner's part
    return table


def status_of(status, index):
    if index < 0:
        return 0                                        # the cell has no device-decoded file
    return int(status[index]) if index < len(status) else BAD_DESC


def decode_mask(status, cell_index, start_index, clip_of, n_clips, dead, active, table):
    """Changes dead [B], active [T,B] and table [n_clips, HEAD] in place."""
    T, B = active.shape
    for b in range(B):
        c = int(clip_of[b])
        if c < 0 or c >= n_clips:
            continue                                    # a slot without a clip: nothing of it changes
        if start_index[b] >= 0:
            s = status_of(status, int(start_index[b]))
            dead[b] = 1 if s != 0 else 0
            table[c, START_STATUS] = s
        for t in range(T):
            if not active[t, b]:
                continue
            s = status_of(status, int(cell_index[t, b]))
            if dead[b]:
                active[t, b] = 0
                table[c, MASKED] += 1
            elif s != 0:
                active[t, b] = 0
                if table[c, FIRST_FAILED] < 0:
                    table[c, FIRST_FAILED] = table[c, DECODED] + table[c, FAILED] + table[c, MASKED]
                    table[c, FIRST_STATUS] = s
                table[c, FAILED] += 1
            else:
                table[c, DECODED] += 1
