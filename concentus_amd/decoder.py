"""Host-side mirror of the reference's decoder API for the CELT-only path.

The reference decodes one stream at a time: opus_decoder_create() -> opus_decode() per packet
(opus-fix/include/opus.h:438-462, src/opus_decoder.c:121,758). `OpusDecoderBatch` keeps the same verbs over N
streams whose state (overlap/history buffer, band energies, post-filter) lives in HBM; all computation happens
in libopusgpu.so (opusgpu_decode_batch; opusgpu_decode_batch_plc when lost packets are to be concealed; opusgpu_decode_batch_any
when the packets may be shorter than 20 ms; opusgpu_decode_batch_packets when they may hold several frames)."""
from . import lib as _lib

OPUS_GET_FINAL_RANGE_REQUEST = 4031
PACKET_FRAMES_BYTES = 200          # sizeof(opusgpu_packet_frames): ret, frame_samples, toc, pad_, offset[48], size[48]


class OpusDecoderBatch:
    """N decoders created alike; decode() consumes the next packet of every stream."""

    def __init__(self, n_streams, Fs=48000, channels=2, device="cuda"):
        import torch
        if Fs != 48000 or channels != 2:
            raise _lib.OpusGpuError(-5, "opus_decoder_create: only 48 kHz stereo is implemented")
        self.n = n_streams
        L = _lib.load()
        self._states = torch.empty((n_streams, L.opusgpu_celt_dec_state_size()), dtype=torch.uint8, device=device)
        self.reset()
        self.final_range = None
        self._frames = None            # decode_packets' frame tables (opusgpu_packet_frames per stream), allocated on first use

    def reset(self):
        """OPUS_RESET_STATE for every stream."""
        _lib.check(_lib.load().opusgpu_celt_dec_state_init(self._states.data_ptr(), self.n, _lib.current_stream_handle()),
                   "opusgpu_celt_dec_state_init")

    def decode(self, packets, lengths, conceal=False, any_frame_size=False, out=None):
        """opus_decode(dec, data, len, pcm, 960, 0) for every stream: packets uint8 [N][stride], lengths int32 [N].
        Returns (pcm int16 [N][960][2], ret int32 [N] = 960 or a negative error per stream).
        Accepted are CELT-only 20 ms single-frame packets, mono or stereo, NB / WB / SWB / FB (TOC 0x98 0xB8 0xD8 0xF8 /
        0x9C 0xBC 0xDC 0xFC), in any mix over the streams and over time; a mono packet comes out on both channels. Any other
        TOC gives that stream -5.
        conceal=True (opusgpu_decode_batch_plc): a stream with length 0 lost its packet and is concealed
        (opus_decode(dec, NULL, 0, ...)) within the bandwidth of its last packet, as is a one-byte DTX packet with one of
        those TOCs, whose bandwidth the stream takes first; its ret is 960 and its final range 0.
        any_frame_size=True (opusgpu_decode_batch_any; implies conceal): frames of 2.5, 5, 10 and 20 ms, the 32 TOCs
        0x80 | bw << 5 | fs << 3 | stereo << 2. ret is then 120, 240, 480 or 960, and only the first ret sample pairs of a
        stream's row of pcm are written (out: a tensor [N][960][2] to write into instead of a fresh uninitialised one). A
        one- or two-byte packet with a short-frame TOC gives -5 (see include/opusgpu.h)."""
        import torch
        if packets.dtype != torch.uint8 or packets.dim() != 2 or packets.shape[0] != self.n or not packets.is_contiguous():
            raise ValueError("packets must be a contiguous uint8 tensor [streams][stride]")
        if lengths.dtype != torch.int32 or lengths.shape != (self.n,):
            raise ValueError("lengths must be int32 [streams]")
        if out is None:
            pcm = torch.empty((self.n, 960, 2), dtype=torch.int16, device=packets.device)
        else:
            if out.dtype != torch.int16 or out.shape != (self.n, 960, 2) or not out.is_contiguous() or out.device != packets.device:
                raise ValueError("out must be a contiguous int16 tensor [streams][960][2] on the packets' device")
            pcm = out
        ret = torch.empty((self.n,), dtype=torch.int32, device=packets.device)
        rng = torch.empty((self.n,), dtype=torch.int32, device=packets.device)
        L = _lib.load()
        name = "opusgpu_decode_batch_any" if any_frame_size else "opusgpu_decode_batch_plc" if conceal else "opusgpu_decode_batch"
        rc = getattr(L, name)(self._states.data_ptr(), packets.data_ptr(), packets.shape[1], lengths.data_ptr(),
                              pcm.data_ptr(), ret.data_ptr(), rng.data_ptr(), self.n, _lib.current_stream_handle())
        _lib.check(rc, name)
        self.final_range = rng
        return pcm, ret

    def decode_packets(self, packets, lengths, frame_size=5760, max_frames=48, out=None):
        """opus_decode(dec, data, len, pcm, frame_size, 0) for every stream (opusgpu_decode_batch_packets): CELT-only packets of any
        frame-count code -- one frame, two, or 1..48 with or without padding --, the 32 TOCs of decode(any_frame_size=True); a
        frame of at most one byte is a DTX frame and is concealed for the TOC's duration.
        Returns (pcm int16 [N][frame_size][2], ret int32 [N]): ret is count * frame_samples, the sample pairs written to the
        stream's row (the rest is left alone; out: a tensor [N][frame_size][2] to write into), 960 for a lost packet (length 0,
        concealed), or -4 for a malformed packet, -2 where the packet is longer than frame_size, -5 for SILK / hybrid TOCs and
        for more than max_frames frames. max_frames (1..48) is how many frame passes are launched: the frame counts stay on
        the device. A rejected stream keeps its state."""
        import torch
        if packets.dtype != torch.uint8 or packets.dim() != 2 or packets.shape[0] != self.n or not packets.is_contiguous():
            raise ValueError("packets must be a contiguous uint8 tensor [streams][stride]")
        if lengths.dtype != torch.int32 or lengths.shape != (self.n,):
            raise ValueError("lengths must be int32 [streams]")
        if out is None:
            pcm = torch.empty((self.n, frame_size, 2), dtype=torch.int16, device=packets.device)
        else:
            if out.dtype != torch.int16 or out.shape != (self.n, frame_size, 2) or not out.is_contiguous() or out.device != packets.device:
                raise ValueError("out must be a contiguous int16 tensor [streams][frame_size][2] on the packets' device")
            pcm = out
        if self._frames is None:
            self._frames = torch.empty((self.n, PACKET_FRAMES_BYTES), dtype=torch.uint8, device=self._states.device)
        ret = torch.empty((self.n,), dtype=torch.int32, device=packets.device)
        rng = torch.empty((self.n,), dtype=torch.int32, device=packets.device)
        rc = _lib.load().opusgpu_decode_batch_packets(self._states.data_ptr(), packets.data_ptr(), packets.shape[1], lengths.data_ptr(),
                                                      pcm.data_ptr(), frame_size, max_frames, self._frames.data_ptr(), ret.data_ptr(),
                                                      rng.data_ptr(), self.n, _lib.current_stream_handle())
        _lib.check(rc, "opusgpu_decode_batch_packets")
        self.final_range = rng
        return pcm, ret

    def decode_lost(self):
        """opus_decode(dec, NULL, 0, pcm, 960, 0) for every stream: all of them lost their packet. Returns (pcm, ret) as decode()."""
        import torch
        dev = self._states.device
        pcm = torch.empty((self.n, 960, 2), dtype=torch.int16, device=dev)
        ret = torch.empty((self.n,), dtype=torch.int32, device=dev)
        rng = torch.empty((self.n,), dtype=torch.int32, device=dev)
        rc = _lib.load().opusgpu_decode_batch_plc(self._states.data_ptr(), None, 0, None, pcm.data_ptr(), ret.data_ptr(),
                                                  rng.data_ptr(), self.n, _lib.current_stream_handle())
        _lib.check(rc, "opusgpu_decode_batch_plc")
        self.final_range = rng
        return pcm, ret

    def ctl(self, request):
        if request == OPUS_GET_FINAL_RANGE_REQUEST:
            return self.final_range
        raise _lib.OpusGpuError(-5, "opus_decoder_ctl request %d" % request)


def decode_independent(packets, lengths, any_frame_size=False):
    """Decode every packet with its own fresh decoder (the first packet of its own stream); the packets may differ in
    channel count and bandwidth (the TOCs of OpusDecoderBatch.decode), with any_frame_size=True in frame size too."""
    dec = OpusDecoderBatch(packets.shape[0], device=packets.device)
    pcm, ret = dec.decode(packets, lengths, any_frame_size=any_frame_size)
    return pcm, ret, dec.final_range


def packet_parse_batch(packets, lengths):
    """opus_packet_parse() for every row of packets uint8 [N][stride] with lengths int32 [N] (opusgpu_packet_parse_batch).
    Returns a dict of tensors: ret int32 [N] (the frame count 1..48, 0 for length 0, -4 for a malformed packet, -1 for a length
    outside the row), frame_samples int16 [N], toc uint8 [N], offset and size int16 [N][48] (of frame f from the start of the
    packet; zero from frame ret on)."""
    import torch
    if packets.dtype != torch.uint8 or packets.dim() != 2 or not packets.is_contiguous():
        raise ValueError("packets must be a contiguous uint8 tensor [streams][stride]")
    n = packets.shape[0]
    if lengths.dtype != torch.int32 or lengths.shape != (n,):
        raise ValueError("lengths must be int32 [streams]")
    rec = torch.empty((n, PACKET_FRAMES_BYTES), dtype=torch.uint8, device=packets.device)
    _lib.check(_lib.load().opusgpu_packet_parse_batch(packets.data_ptr(), packets.shape[1], lengths.data_ptr(), rec.data_ptr(), n,
                                                      _lib.current_stream_handle()), "opusgpu_packet_parse_batch")
    i16 = rec[:, 4:].contiguous().view(torch.int16)           # frame_samples, (toc, pad_), offset[48], size[48]
    return {"ret": rec[:, :4].contiguous().view(torch.int32).reshape(n).clone(), "frame_samples": i16[:, 0].clone(), "toc": rec[:, 6].clone(),
            "offset": i16[:, 2:50].clone(), "size": i16[:, 50:98].clone()}
