"""What the host tests of the packed MX KV cache (test_kv_packed*_host.py) share: msq.kvpacked.PackedKV and StaticPackedKV with their storage on
the host and logs instead of launches, so that the timing rule and the host mirror run as plain Python."""
import torch


def _msq():
    import msq
    msq._lib.lib()
    return msq


def _tokens(a, b):
    """k, v [1, 1, b - a, 32]: token i holds the value i"""
    t = torch.arange(a, b, dtype=torch.float16).reshape(1, 1, -1, 1).expand(1, 1, b - a, 32).contiguous()
    return t, t.clone()


class _PackLog:
    """_pack records (pos, the tokens' values) in `log`; with keep_tokens it also keeps the tokens in `store`, and _unpack hands them back and
    records (pos, T) in `unpacks`"""
    keep_tokens = False

    def _check_device(self):
        pass

    def _check_kv(self, k, v):
        pass

    def _pack(self, k, v, pos):
        assert k.shape == v.shape and k.shape[2] % 32 == 0 and pos % 32 == 0 and pos + k.shape[2] <= self.capacity
        self.log.append((pos, k[0, 0, :, 0].tolist()))
        if self.keep_tokens:
            for i in range(k.shape[2]):
                self.store[pos + i] = (k[:, :, i].clone(), v[:, :, i].clone())

    def _unpack(self, pos, T):
        if not self.keep_tokens:
            return super()._unpack(pos, T)
        self.unpacks.append((pos, T))
        return (torch.stack([self.store[pos + i][0] for i in range(T)], dim=2), torch.stack([self.store[pos + i][1] for i in range(T)], dim=2))


def dynamic_stub(gap, keep_tokens=False):
    class Stub(_PackLog, _msq().kvpacked.PackedKV):
        def _reserve(self, need):
            self.capacity = max(self.capacity, (need + 31) // 32 * 32)

    Stub.keep_tokens = keep_tokens
    s = Stub(1, 1, 32, torch.float16, "fp8_e4m3", gap=gap, capacity=32, device="cpu")
    s.log, s.store, s.unpacks = [], {}, []
    return s


def static_stub(gap, max_len, keep_tokens=False):
    class Stub(_PackLog, _msq().kvpacked.StaticPackedKV):
        """the device state is a list that _append_dev moves by the rule of include/msq.h (the kernels' side of the contract, restated), so
        that sync() can be compared with the mirror"""
        def _alloc_planes(self):
            self.planes, self.capacity = {}, self.S_cap

        def _alloc_state(self):
            self.dev, self.writes, self.launches, self.capturing = [0, 0, 0, 0], 0, 0, False

        def _write_state(self, clear_status=False):
            self.dev[:2] = [self.packed_len, self.tail_len]
            if clear_status:
                self.dev[2] = 0
            self.writes += 1

        def _read_state(self):
            return list(self.dev)

        def _capturing(self):
            return self.capturing

        def _append_dev(self, k, v):
            self.launches += 1
            p, t = self.dev[:2]
            if t == self.gap:
                if p + self.gap > self.S_cap:
                    self.dev[2] |= 8
                    return
                self.log.append((p, self.k_tail[0, 0, :, 0].tolist()))
                p, t = p + self.gap, 0
            self.k_tail[:, :, t:t + 1] = k
            self.v_tail[:, :, t:t + 1] = v
            self.dev[:2] = [p, t + 1]

    Stub.keep_tokens = keep_tokens
    s = Stub(1, 1, 32, torch.float16, "fp8_e4m3", gap=gap, max_len=max_len, device="cpu")
    s.log, s.store, s.unpacks = [], {}, []
    return s
