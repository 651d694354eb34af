"""Piece sizes shared by tests/test_ips_stream_cpu.py and tests/test_ips_stream.py."""


def piece_patterns(N, M, I):
    """Piece sizes that never align with the chunks (each list sums to N): all ones, a first piece shorter than M, a first
    piece longer than M + 2 I, 3.5 chunks at once, the whole input."""
    def fill(first, step):
        out, left = [], N
        for n in first:
            n = min(n, left)
            if n:
                out.append(n)
                left -= n
        while left:
            out.append(min(step, left))
            left -= out[-1]
        return out
    return {"ones": [1] * N,
            "short_first": fill([max(1, M - 3)], I + 1),
            "long_first": fill([M + 2 * I + 1], max(1, I - 1)),
            "chunks3p5": fill([], 3 * I + max(1, I // 2)),
            "whole": [N]}
