# SLAMHipStreams.jl -- the throughput path of libslamhip.so for a Julia host: S lock-stepped camera streams whose pyramids are
# built in one launch set per step and whose keypoint lists never leave HBM (include/slamhip.h, "lock-stepped batches of
# streams" and "device-resident keypoint lists"; DESIGN.md 3.10; INTEGRATION.md has the per-frame call sequence).
#
# SLAMHip.jl rebinds the reference's own seams one call at a time (one stream, host arrays in and out).  This file is what a
# host that runs many sequences at once -- the configuration the bench line is quoted on -- binds instead: the same C entry
# points Python's slam.jl_amd.PyramidBatch / KeypointSet wrap.  Device memory for the frames comes from the HIP runtime
# directly (hipMalloc / hipMemcpyAsync on the context's stream): no AMDGPU.jl, no Julia GPU codegen.
#
#     include("SLAMHip.jl"); include("SLAMHipStreams.jl")
#     SLAMHip.activate!("/path/to/libslamhip.so")
#     using .SLAMHipStreams
#     left = PyramidBatch(H, W, 3, S); prev = PyramidBatch(H, W, 3, S)
#     frames = FrameRing(H, W, S)                       # S uint8 frames in HBM + a pinned staging buffer
#     ks = KeypointSet(S, 2048)
#     upload!(frames, images_u8)                        # Vector of S Matrix{UInt8} (column-major H x W, KITTI decode)
#     update!(left, frames)                             # slam_pyr_update_batch_u8_dev
#     flow_match!(ks, prev, left, params; prior = 1)    # klt_tracking! for every stream
#     ...
#
# NOTE: like SLAMHip.jl, written against the Julia manual and include/slamhip.h, never executed (no Julia in the build
# container).  Every ccall mirrors the prototype of the same name in include/slamhip.h, argument for argument, so that a maintainer
# can check it by inspection.
module SLAMHipStreams

import ..SLAMHip: LIB, ctx, check

export update_selected!
export PyramidBatch, FrameRing, KeypointSet, upload!, update!, flow_match!, stereo_match!, remove!, detect!, detect_describe!, describe_batch, keyframe!, select!, selection,
       triangulate!, triangulate_lens!, upload_stereo!, triangulate_temporal!, compute_pose_5pt!, compute_pose!, frame_stats, keyframe_required, counts, download, stream_params,
       KeyframeMap, add_keyframe!, gather, download_keyframe, download_points, reset!, filter_map!, remove_keyframe!, newest, enable_pixels!, keyframe_pixels

const HIP = "libamdhip64"
hipcheck(e::Cint, what) = e == 0 || error("$what: HIP error $e")

# ---- S pyramids in one allocation (slamhip.h: slam_pyr_create_batch) ---------------------------------------------------------
mutable struct PyramidBatch
    handles::Vector{Ptr{Cvoid}}          # the S members: ordinary slam_pyr handles (member 1 stands for the batch in the match calls)
    H::Int; W::Int; levels::Int
    function PyramidBatch(H, W, levels, S)
        hs = fill(C_NULL, S)
        check(ccall((:slam_pyr_create_batch, LIB[]), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Ptr{Cvoid}}), ctx(), H, W, levels, S, hs))
        b = new(hs, H, W, levels)
        finalizer(x -> foreach(h -> ccall((:slam_pyr_destroy, LIB[]), Cint, (Ptr{Cvoid},), h), x.handles), b)   # plain C calls: no locks, no task switches
        b
    end
end
Base.length(b::PyramidBatch) = length(b.handles)

# ---- S uint8 frames in HBM, filled from the host through a pinned buffer on the context's stream ------------------------------
mutable struct FrameRing
    dev::Ptr{UInt8}; pinned::Ptr{UInt8}; ptrs::Vector{Ptr{UInt8}}; H::Int; W::Int; S::Int
    function FrameRing(H, W, S)
        d = Ref{Ptr{Cvoid}}(C_NULL); p = Ref{Ptr{Cvoid}}(C_NULL)
        hipcheck(ccall((:hipMalloc, HIP), Cint, (Ref{Ptr{Cvoid}}, Csize_t), d, H * W * S), "hipMalloc")
        hipcheck(ccall((:hipHostMalloc, HIP), Cint, (Ref{Ptr{Cvoid}}, Csize_t, Cuint), p, H * W * S, 0), "hipHostMalloc")
        f = new(Ptr{UInt8}(d[]), Ptr{UInt8}(p[]), [Ptr{UInt8}(d[]) + (s - 1) * H * W for s in 1:S], H, W, S)
        finalizer(x -> (ccall((:hipFree, HIP), Cint, (Ptr{Cvoid},), x.dev); ccall((:hipHostFree, HIP), Cint, (Ptr{Cvoid},), x.pinned)), f)
        f
    end
end

"frames: S matrices of UInt8 (H x W, column-major as Julia stores them).  Asynchronous on the context's stream; the pinned buffer
is reused by the next call, which therefore waits for this copy (slam_ctx_synchronize) first."
function upload!(f::FrameRing, frames::AbstractVector{<:AbstractMatrix{UInt8}})
    length(frames) == f.S || error("expected $(f.S) frames")
    check(ccall((:slam_ctx_synchronize, LIB[]), Cint, (Ptr{Cvoid},), ctx()))
    n = f.H * f.W
    for (s, img) in enumerate(frames)
        size(img) == (f.H, f.W) || error("frame $s has size $(size(img))")
        GC.@preserve img unsafe_copyto!(f.pinned + (s - 1) * n, pointer(img), n)
    end
    stream = ccall((:slam_ctx_stream, LIB[]), Ptr{Cvoid}, (Ptr{Cvoid},), ctx())
    hipcheck(ccall((:hipMemcpyAsync, HIP), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint, Ptr{Cvoid}), f.dev, f.pinned, n * f.S, 1, stream), "hipMemcpyAsync")   # 1 = hipMemcpyHostToDevice
    f
end

"update! of all S pyramids from the uint8 frames (raw / 255 on the device; slamhip.h: slam_pyr_update_batch_u8_dev).  target_only:
the batch is only ever matched INTO (right pyramids, mapper.jl:51-66) -- SLAM_PYR_TARGET_ONLY = 16.  tolerance = true selects mode 3:
with S >= 4 the tolerance-mode batch build (every plane within 1e-11 of the bit-exact one relative to the plane's magnitude, 2.2x instead
of 3.9x the algorithmic bytes; keypoint indices unaffected -- detect! works on the base layer); the default is the bit-exact mode 1."
function update!(b::PyramidBatch, f::FrameRing; σ = 1.0, target_only::Bool = false, tolerance::Bool = false, sync::Bool = false)
    hs = b.handles; ps = f.ptrs
    mode = (tolerance ? 3 : 1) | (target_only ? 16 : 0)
    GC.@preserve hs ps check(ccall((:slam_pyr_update_batch_u8_dev, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{UInt8}}, Cint, Cint, Cdouble, Cint),
        ctx(), hs, ps, length(hs), mode, Float64(σ), sync ? 1 : 0))
    b
end

"The COMPACT build (slamhip.h: slam_pyr_update_batch_sel_u8_dev): member r of `b` receives the build of the r-th selected stream of the ring,
ascending; members at index n_sel or above keep their bytes.  selected: one entry per stream of the ring (Bool or UInt8; the `required` of
keyframe_required as it is) or nothing = every stream.  `b` may have fewer members than the ring has streams; more selected streams than members is
an error.  The batch remembers the mask: stereo_match!(...; compact = true) refuses it under any other selection.  Returns n_sel."
function update_selected!(b::PyramidBatch, f::FrameRing, selected; σ = 1.0, target_only::Bool = false, tolerance::Bool = false, sync::Bool = false)
    hs = b.handles; ps = f.ptrs
    mode = (tolerance ? 3 : 1) | (target_only ? 16 : 0)
    m = selected ≡ nothing ? nothing : UInt8[x != 0 ? 0x01 : 0x00 for x in selected]
    m ≡ nothing || length(m) == f.S || error("expected $(f.S) mask entries")
    n = Ref{Cint}(0)
    GC.@preserve hs ps m check(ccall((:slam_pyr_update_batch_sel_u8_dev, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Cint, Ptr{Ptr{UInt8}}, Cint, Ptr{UInt8}, Cint, Cdouble, Cint, Ref{Cint}),
        ctx(), hs, length(hs), ps, f.S, m ≡ nothing ? C_NULL : pointer(m), mode, Float64(σ), sync ? 1 : 0, n))
    Int(n[])
end

# ---- per-stream call parameters (slamhip.h: S x 32 doubles) ---------------------------------------------------------------------
"params[:, s] = [Tcw (column-major 4 x 4) ; fx fy cx cy ; k1 k2 p1 p2 ; shift_y shift_x ; 0 ...]"
function stream_params(S; Tcw = nothing, cam = (1.0, 1.0, 0.0, 0.0), dist = (0.0, 0.0, 0.0, 0.0), shift = (0.0, 0.0))
    p = zeros(Float64, 32, S)
    for s in 1:S
        T = Tcw ≡ nothing ? [1.0 0 0 0; 0 1 0 0; 0 0 1 0; 0 0 0 1] : (Tcw isa AbstractVector ? Tcw[s] : Tcw)
        p[1:16, s] .= vec(Matrix{Float64}(T)); p[17:20, s] .= cam; p[21:24, s] .= dist; p[25:26, s] .= shift
    end
    p
end

# ---- the keypoint lists of S streams in HBM (slamhip.h: slam_kpset_*) -----------------------------------------------------------
mutable struct KeypointSet
    h::Ptr{Cvoid}; S::Int; cap::Int
    function KeypointSet(S, cap)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_kpset_create, LIB[]), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}), ctx(), S, cap, r))
        k = new(r[], S, cap)
        finalizer(x -> ccall((:slam_kpset_destroy, LIB[]), Cint, (Ptr{Cvoid},), x.h), k)
        k
    end
end

"replace stream s's list (1-based s): yx 2 x n (y, x), is_3d n, xyz 3 x n"
function upload!(k::KeypointSet, s, yx::Matrix{Float64}, is_3d::Vector{UInt8}, xyz::Matrix{Float64})
    n = size(yx, 2)
    GC.@preserve yx is_3d xyz check(ccall((:slam_kpset_upload, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Cint),
        ctx(), k.h, s - 1, yx, is_3d, xyz, C_NULL, n))
    k
end

function download(k::KeypointSet, s)
    yx = zeros(2, k.cap); is3 = zeros(UInt8, k.cap); xyz = zeros(3, k.cap); ids = zeros(Int64, k.cap)
    syx = zeros(2, k.cap); hs = zeros(UInt8, k.cap); n = Ref{Cint}(0)
    check(ccall((:slam_kpset_download, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}, Cint, Ref{Cint}),
        ctx(), k.h, s - 1, yx, is3, xyz, ids, syx, hs, k.cap, n))
    m = Int(n[])
    (yx = yx[:, 1:m], is_3d = is3[1:m] .!= 0, xyz = xyz[:, 1:m], ids = ids[1:m], stereo_yx = syx[:, 1:m], has_stereo = hs[1:m] .!= 0)
end

"the S list lengths: the one small device -> host copy of a step that ends without compute_pose!"
function counts(k::KeypointSet)
    c = zeros(Int32, k.S)
    check(ccall((:slam_kpset_counts, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}), ctx(), k.h, c))
    c
end

# optical_flow_matching!(map_manager, frame, from, to, false) for every stream (map_manager.jl:451-564)
function flow_match!(k::KeypointSet, from::PyramidBatch, to::PyramidBatch, params::Matrix{Float64}; prior = 0, pyramid_levels = 3,
                     pyramid_levels_3d = 1, window = 9, iterations = 30, eig_thr = 1e-4, eps = 0.01, max_distance = 1.0, n_bound = 0)   # max_distance = params.max_ktl_distance
    GC.@preserve params check(ccall((:slam_kpset_flow_match, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Cint, Cint, Cint, Cdouble, Cdouble, Cdouble, Cint),
        ctx(), k.h, from.handles[1], to.handles[1], params, prior, pyramid_levels, pyramid_levels_3d, window, iterations,
        eig_thr, eps, max_distance, n_bound))
    k
end

# optical_flow_matching!(..., true) + maybe_stereo_update! (map_manager.jl:579-590); params: the RIGHT camera
function stereo_match!(k::KeypointSet, left::PyramidBatch, right::PyramidBatch, params::Matrix{Float64}; prior = 2, pyramid_levels = 3,
                       pyramid_levels_3d = 1, window = 9, iterations = 30, eig_thr = 1e-4, eps = 0.01, max_distance = 1.0,
                       epipolar_error = 2.0, n_bound = 0, compact::Bool = false)
    # compact: `right` is a compact batch (update_selected! under the set's current selection): stream s's target is its member rank(s)
    if compact
        GC.@preserve params check(ccall((:slam_kpset_stereo_match_compact, LIB[]), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Cint, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Cint),
            ctx(), k.h, left.handles[1], right.handles[1], params, prior, pyramid_levels, pyramid_levels_3d, window, iterations,
            eig_thr, eps, max_distance, epipolar_error, n_bound))
        return k
    end
    GC.@preserve params check(ccall((:slam_kpset_stereo_match, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Cint, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Cint),
        ctx(), k.h, left.handles[1], right.handles[1], params, prior, pyramid_levels, pyramid_levels_3d, window, iterations,
        eig_thr, eps, max_distance, epipolar_error, n_bound))
    k
end

"flags_dev: S x cap bytes in HBM (slot order), e.g. written by the host's own culling kernel or uploaded with hipMemcpy"
remove!(k::KeypointSet, flags_dev::Ptr{UInt8}) = (check(ccall((:slam_kpset_remove, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}), ctx(), k.h, flags_dev)); k)

# extract_keypoints! (map_manager.jl:98-113): e is the reference's Extractor (max_points, radius, grid_resolution, cell_size)
function detect!(k::KeypointSet, cur::PyramidBatch, e; σ_mask = 3.0, min_response = 1e-4)
    check(ccall((:slam_kpset_detect, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cdouble, Cdouble),
        ctx(), k.h, cur.handles[1], e.max_points, e.radius, e.grid_resolution[1], e.grid_resolution[2], e.cell_size, Float64(σ_mask), min_response))
    k
end

# extract_keypoints! with describe (map_manager.jl:98-113): as detect!, but the candidates describe() drops at the border are not appended and
# the appended ones are described.  table: 4 x n_bits Int32 (SLAMHip.brief_table(e)); desc_dev: S x dcap x (n_bits ÷ 64) UInt64 and info_dev:
# S x 2 Int64 in HBM (hipMalloc) -- the j-th keypoint (0-based) this call appends to stream s (0-based) has id info[2 s] + j and its descriptor at
# desc[(s dcap + j) words ..]; info[2 s + 1] keypoints were appended.  dcap ≥ cells * cld(e.max_points, cells).  Enqueue-only.
function detect_describe!(k::KeypointSet, cur::PyramidBatch, e, table::Matrix{Int32}, desc_dev::Ptr{UInt64}, info_dev::Ptr{Int64}, dcap::Integer;
                          σ_mask = 3.0, min_response = 1e-4, σ = sqrt(2.0), window = 9)
    GC.@preserve table check(ccall((:slam_kpset_detect_describe, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Cdouble, Cdouble, Ptr{Int32}, Cint, Cdouble, Cint, Ptr{UInt64}, Ptr{Int64}, Cint),
        ctx(), k.h, cur.handles[1], e.max_points, e.radius, e.grid_resolution[1], e.grid_resolution[2], e.cell_size, Float64(σ_mask), min_response,
        table, size(table, 2), Float64(σ), window, desc_dev, info_dev, dcap))
    k
end

# describe() for every stream of a batch in one launch: rc 2 x n Int64 (row, col) grouped by stream, off S + 1 Int32 (0-based offsets, off[1] = 0).
# Returns (bits words x m, rc 2 x m, out_off S + 1): stream s (1-based) owns the columns out_off[s] + 1 : out_off[s + 1].
function describe_batch(cur::PyramidBatch, rc::Matrix{Int64}, off::Vector{Int32}, table::Matrix{Int32}; σ = sqrt(2.0), window = 9)
    S = length(cur); n = size(rc, 2); words = size(table, 2) ÷ 64
    bits = Matrix{UInt64}(undef, words, n); orc = Matrix{Int64}(undef, 2, n); out_off = zeros(Int32, S + 1)
    GC.@preserve rc off table bits orc out_off check(ccall((:slam_describe_batch, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Cint, Cdouble, Cint, Ptr{UInt64}, Ptr{Int64}, Ptr{Int32}),
        ctx(), cur.handles[1], S, rc, off, table, size(table, 2), Float64(σ), window, bits, orc, out_off))
    m = Int(out_off[S + 1])
    bits[:, 1:m], orc[:, 1:m], out_off
end

# create_keyframe! as far as the lists go (map_manager.jl:60-96); call after detect!
keyframe!(k::KeypointSet) = (check(ccall((:slam_kpset_keyframe, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), k.h)); k)

# The streams the six key-frame seams act on (detect!, detect_describe!, keyframe!, stereo_match!, triangulate!, triangulate_temporal!): mask = S
# entries, non-zero / true = selected (the `required` of keyframe_required as it is), or nothing = every stream.  Every other call acts on all
# streams.  The selection holds until the next select!; the bytes are staged, `mask` is free on return.
function select!(k::KeypointSet, mask::Union{Nothing,AbstractVector})
    if mask === nothing
        check(ccall((:slam_kpset_select, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}), ctx(), k.h, C_NULL))
    else
        length(mask) == k.S || throw(ArgumentError("select!: $(length(mask)) entries for $(k.S) streams"))
        m = UInt8[x != 0 ? 0x01 : 0x00 for x in mask]
        GC.@preserve m check(ccall((:slam_kpset_select, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}), ctx(), k.h, m))
    end
    k
end
"the current selection as S Bools (all true when none is set)"
function selection(k::KeypointSet)
    m = zeros(UInt8, k.S)
    check(ccall((:slam_kpset_selection, LIB[]), Cint, (Ptr{Cvoid}, Ptr{UInt8}), k.h, m))
    m .!= 0
end

# triangulate_stereo! (mapper.jl:142-183): P1, P2 4 x 4 projection matrices, T21 right <- left, cam1 / cam2 = (fx, fy, cx, cy), Twc 16 x S
function triangulate!(k::KeypointSet, P1::Matrix{Float64}, P2::Matrix{Float64}, T21::Matrix{Float64}, cam1, cam2, Twc::Matrix{Float64};
                      max_error = 3.0, min_depth = 0.1, n_bound = 0)
    c1 = collect(Float64, cam1); c2 = collect(Float64, cam2)
    GC.@preserve P1 P2 T21 c1 c2 Twc check(ccall((:slam_kpset_triangulate, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint),
        ctx(), k.h, P1, P2, T21, c1, c2, Twc, max_error, min_depth, n_bound))
    k
end

# The same for a rig with lenses: dist1 / dist2 = (k1, k2, p1, p2) of the left / right camera; both pixels are undistorted, each through its own
# camera, before the DLT and the gates (slam_kpset_triangulate_lens).  The lists keep the raw pixels.
function triangulate_lens!(k::KeypointSet, P1::Matrix{Float64}, P2::Matrix{Float64}, T21::Matrix{Float64}, cam1, cam2, dist1, dist2, Twc::Matrix{Float64};
                           max_error = 3.0, min_depth = 0.1, n_bound = 0)
    c1 = collect(Float64, cam1); c2 = collect(Float64, cam2); d1 = collect(Float64, dist1); d2 = collect(Float64, dist2)
    GC.@preserve P1 P2 T21 c1 c2 d1 d2 Twc check(ccall((:slam_kpset_triangulate_lens, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cdouble, Cdouble, Cint),
        ctx(), k.h, P1, P2, T21, c1, c2, d1, d2, Twc, max_error, min_depth, n_bound))
    k
end
# the stereo observations of stream s's list (1-based s, as upload! and download; restoring state): stereo_yx 2 x n (y, x) in the right image,
# has_stereo n flags
function upload_stereo!(k::KeypointSet, s, stereo_yx::Matrix{Float64}, has_stereo::Vector{UInt8})
    n = length(has_stereo)
    size(stereo_yx) == (2, n) || error("upload_stereo!: stereo_yx is $(size(stereo_yx)), has_stereo has $n flags")
    GC.@preserve stereo_yx has_stereo check(ccall((:slam_kpset_upload_stereo, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{UInt8}, Cint),
        ctx(), k.h, s - 1, stereo_yx, has_stereo, n))
    k
end

# triangulate_temporal! (mapper.jl:185-262).  kf_cw[s][q]: world -> camera of key-frame id q' with q' % nkf == q - 1 (a ring of the last
# nkf key-frame poses), Twc[s]: camera -> world of the frame, K4: the 4 x 4 calibration matrix; the four matrices per observer are the
# ones mapper.jl:226-231 forms.
function triangulate_temporal!(k::KeypointSet, params::Matrix{Float64}, kf_cw, Twc, K4::Matrix{Float64}, kf_cur::Vector{Int32};
                               kf_lo = nothing, max_error = 3.0, min_depth = 0.1, min_parallax = 20.0, n_bound = 0)
    nkf = length(kf_cw[1])
    tab = zeros(Float64, 64, nkf, k.S)
    for s in 1:k.S, q in 1:nkf
        rel = kf_cw[s][q] * Twc[s]; rel_inv = inv(rel)
        tab[1:16, q, s] .= vec(K4 * rel_inv); tab[17:32, q, s] .= vec(rel_inv); tab[33:48, q, s] .= vec(rel); tab[49:64, q, s] .= vec(inv(kf_cw[s][q]))
    end
    lo = kf_lo ≡ nothing ? Int32.(max.(kf_cur .- (nkf - 1), 0)) : kf_lo
    GC.@preserve params tab kf_cur lo check(ccall((:slam_kpset_triangulate_temporal, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Int32}, Ptr{Int32}, Cdouble, Cdouble, Cdouble, Cint),
        ctx(), k.h, params, tab, nkf, kf_cur, lo, max_error, min_depth, min_parallax, n_bound))
    k
end

# compute_pose_5pt! (front_end.jl:242-332): params[1:9, s] = R_compensation (column-major 3 x 3), [17:24] camera + distortion.
# fetch = false: enqueue only (the epipolar filter acts on the lists; compute_pose! right behind it brings the step's copy).
function compute_pose_5pt!(k::KeypointSet, params::Matrix{Float64}; min_parallax = 5.0, max_repr_error = 3.0, iters = 128, seed = UInt64(0), fetch = true)
    if !fetch
        GC.@preserve params check(ccall((:slam_kpset_compute_pose_5pt, LIB[]), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cdouble, Cdouble, Cint, UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
            ctx(), k.h, params, min_parallax, max_repr_error, iters, seed, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
        return nothing
    end
    P = zeros(Float64, 12, k.S); status = zeros(Int32, k.S); ninl = zeros(Int32, k.S); par = zeros(Float64, k.S); cnt = zeros(Int32, k.S)
    GC.@preserve params check(ccall((:slam_kpset_compute_pose_5pt, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cdouble, Cdouble, Cint, UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
        ctx(), k.h, params, min_parallax, max_repr_error, iters, seed, P, status, ninl, par, cnt))
    (Rt = [reshape(P[:, s], 3, 4) for s in 1:k.S], status = status, n_inliers = ninl, parallax = par, counts = cnt)
end

# What check_new_kf_required (flags = 1) / check_ready_for_init! (flags = 2) read of the frame (slam_kpset_frame_stats): an 8 x S matrix, per
# stream [list length, nb_3d_kpts, nb_stereo_kpts, keypoints the key-frame observes, nb_occupied_cells, n_parallax, mean, median parallax].
# params as for compute_pose_5pt!.  fetch = false: enqueue only; the results stay in HBM (stats_dev, or a buffer of the set).
function frame_stats(k::KeypointSet, params::Matrix{Float64}, flags::Integer, cell_size::Integer, height::Integer, width::Integer;
                     fetch = true, stats_dev::Ptr{Cvoid} = C_NULL)
    if !fetch
        GC.@preserve params check(ccall((:slam_kpset_frame_stats, LIB[]), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Float64}),
            ctx(), k.h, params, flags, cell_size, height, width, stats_dev, C_NULL))
        return nothing
    end
    stats = zeros(Float64, 8, k.S)
    GC.@preserve params check(ccall((:slam_kpset_frame_stats, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Float64}),
        ctx(), k.h, params, flags, cell_size, height, width, stats_dev, stats))
    stats
end

# check_new_kf_required (front_end.jl:361-393) per stream on those statistics (slam_keyframe_required: host arithmetic, no device).
# prev_kf_nb_3d: the key-frames' own nb_3d_kpts (the mapper and the estimator change it: the caller owns it).  rule: which exit decided.
function keyframe_required(stats::Matrix{Float64}, frames_delta::Vector{Int32}, prev_kf_nb_3d::Vector{Int32}, has_prev_kf::Vector{UInt8};
                           max_nb_keypoints::Integer, initial_parallax::Real = 20.0, local_ba_on::Bool = false)
    S = size(stats, 2)
    required = zeros(UInt8, S); rule = zeros(UInt8, S)
    check(ccall((:slam_keyframe_required, LIB[]), Cint,
        (Cint, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}, Cint, Cdouble, Cint, Ptr{UInt8}, Ptr{UInt8}),
        S, stats, frames_delta, prev_kf_nb_3d, has_prev_kf, max_nb_keypoints, Float64(initial_parallax), local_ba_on ? 1 : 0, required, rule))
    (required = required .!= 0, rule = rule)
end

# compute_pose! (front_end.jl:132-219): P3P RANSAC + pnp_bundle_adjustment on the lists; the step's device -> host copy
function compute_pose!(k::KeypointSet, params::Matrix{Float64}; threshold = 3.0, iters = 256, seed = UInt64(0), pnp_iters_fast = 5,
                       pnp_iterations = 10, depth_eps = 1e-6, repr_eps = threshold)
    poses = zeros(Float64, 16, k.S); status = zeros(Int32, k.S); ninl = zeros(Int32, k.S); cnt = zeros(Int32, k.S)
    GC.@preserve params check(ccall((:slam_kpset_compute_pose, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cdouble, Cint, UInt64, Cint, Cint, Cdouble, Cdouble, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
        ctx(), k.h, params, threshold, iters, seed, pnp_iters_fast, pnp_iterations, depth_eps, repr_eps, poses, status, ninl, cnt))
    (Tcw = [reshape(poses[:, s], 4, 4) for s in 1:k.S], status = status, n_inliers = ninl, counts = cnt)
end

# bundle_adjustment! (bundle_adjustment.jl:1-111) for the LocalBACaches of S lock-stepped SlamManagers in one set of launches
# (slam_local_ba_batch): what the S estimator tasks (estimator.jl:78-99, local_bundle_adjustment! :317-347) would each call once per
# key-frame.  caches: any objects with the LocalBACache fields (θ, θconst, pixels, poses_ids, points_ids, outliers, poses_remap,
# points_remap, observations -- estimator.jl:16-40); cameras: one Camera per cache.  Mutates every cache.θ / cache.outliers like
# S bundle_adjustment! calls; returns the per-window status codes (0 = solved; a window whose reduced system was not positive definite
# is left unchanged and reports -5).
function bundle_adjustment_batch!(caches::AbstractVector, cameras::AbstractVector; iterations::Int = 10, repr_ϵ::Real = 5.0)
    S = length(caches)
    Pn = Int32[length(c.poses_remap) for c in caches]; Mn = Int32[length(c.points_remap) for c in caches]; On = Int32[length(c.observations) for c in caches]
    cams = Float64[]; for cam in cameras; append!(cams, (cam.fx, cam.fy, cam.cx, cam.cy)); end
    θ = reduce(vcat, [Vector{Float64}(c.θ) for c in caches]); tc = reduce(vcat, [Vector{UInt8}(c.θconst) for c in caches])
    px = reduce(vcat, [vec(Matrix{Float64}(c.pixels)) for c in caches])                  # 2 x O column-major = (y, x) pairs back to back
    pid = reduce(vcat, [Vector{Int64}(c.poses_ids) for c in caches]); lid = reduce(vcat, [Vector{Int64}(c.points_ids) for c in caches])
    outl = zeros(UInt8, max(sum(On), 1)); status = zeros(Int32, S)
    GC.@preserve cams Pn Mn On θ tc px pid lid outl status check(ccall((:slam_local_ba_batch, LIB[]), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{UInt8},
         Cint, Cint, Cdouble, Ptr{Float64}, Ptr{Int32}),
        ctx(), S, cams, Pn, Mn, On, θ, tc, px, pid, lid, outl, 5, iterations, Float64(repr_ϵ), C_NULL, status))
    to = 0; oo = 0
    for (z, c) in enumerate(caches)
        n = 6 * Pn[z] + 3 * Mn[z]
        copyto!(c.θ, 1, θ, to + 1, n); to += n
        for i in 1:On[z]; c.outliers[i] = outl[oo + i] != 0; end
        oo += On[z]
    end
    status
end

# The same in two halves (slam_local_ba_batch_begin / _end): `begin` packs the caches and hands the call to a thread of the library -- the
# estimator task goes on (e.g. packs the next key-frame's caches) --, `finish!` waits and writes θ / outliers back.  The packed arrays live in the
# returned job until then; `jctx` is a context of the job's own (one job per context).
struct BABatchJob; jctx::Ptr{Cvoid}; caches; Pn; Mn; On; cams; θ; tc; px; pid; lid; outl; status; end
function bundle_adjustment_batch_begin(jctx::Ptr{Cvoid}, caches::AbstractVector, cameras::AbstractVector; iterations::Int = 10, repr_ϵ::Real = 5.0)
    S = length(caches)
    Pn = Int32[length(c.poses_remap) for c in caches]; Mn = Int32[length(c.points_remap) for c in caches]; On = Int32[length(c.observations) for c in caches]
    cams = Float64[]; for cam in cameras; append!(cams, (cam.fx, cam.fy, cam.cx, cam.cy)); end
    θ = reduce(vcat, [Vector{Float64}(c.θ) for c in caches]); tc = reduce(vcat, [Vector{UInt8}(c.θconst) for c in caches])
    px = reduce(vcat, [vec(Matrix{Float64}(c.pixels)) for c in caches])
    pid = reduce(vcat, [Vector{Int64}(c.poses_ids) for c in caches]); lid = reduce(vcat, [Vector{Int64}(c.points_ids) for c in caches])
    outl = zeros(UInt8, max(sum(On), 1)); status = zeros(Int32, S)
    job = BABatchJob(jctx, caches, Pn, Mn, On, cams, θ, tc, px, pid, lid, outl, status)       # (the job keeps every array alive until finish!)
    check(ccall((:slam_local_ba_batch_begin, LIB[]), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{UInt8},
         Cint, Cint, Cdouble, Ptr{Float64}, Ptr{Int32}),
        jctx, S, cams, Pn, Mn, On, θ, tc, px, pid, lid, outl, 5, iterations, Float64(repr_ϵ), C_NULL, status))
    job
end
function finish!(job::BABatchJob)
    check(ccall((:slam_local_ba_batch_end, LIB[]), Cint, (Ptr{Cvoid},), job.jctx))
    to = 0; oo = 0
    for (z, c) in enumerate(job.caches)
        n = 6 * job.Pn[z] + 3 * job.Mn[z]
        copyto!(c.θ, 1, job.θ, to + 1, n); to += n
        for i in 1:job.On[z]; c.outliers[i] = job.outl[oo + i] != 0; end
        oo += job.On[z]
    end
    job.status
end

# ---- the key-frame map of the lists (slam_kfmap_*, include/slamhip.h): _get_ba_parameters / _update_ba_parameters! (estimator.jl:143-306) for S
# lock-stepped streams whose keypoints live in a KeypointSet.  add_keyframe! right after keyframe!; gather returns the windows of the newest key-frames
# in slam_local_ba_batch's layout (pass the arrays straight on); update! takes θ and the outlier flags back, into the map and (k given) the live lists.
# KfmapWindows mirrors slam_kfmap_windows field for field; the arrays it points to belong to the GatheredWindows that owns it.
mutable struct KfmapWindows
    cap_windows::Int32; cap_poses::Int32; cap_points::Int32; cap_obs::Int32
    status::Ptr{Int32}; win_stream::Ptr{Int32}; Pn::Ptr{Int32}; Mn::Ptr{Int32}; On::Ptr{Int32}
    theta::Ptr{Float64}; theta_const::Ptr{UInt8}; pixels_yx::Ptr{Float64}; pose_ids::Ptr{Int64}; point_ids::Ptr{Int64}
    poses_remap::Ptr{Int64}; points_remap::Ptr{Int64}; obs_kf::Ptr{Int64}; obs_kp::Ptr{Int64}; obs_in_covmap::Ptr{UInt8}
end
mutable struct KeyframeMap
    h::Ptr{Cvoid}; S::Int; cap::Int; R::Int; mcap::Int
    function KeyframeMap(S, cap; R = 32, mcap = 16384)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:slam_kfmap_create, LIB[]), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ref{Ptr{Cvoid}}), ctx(), S, cap, R, mcap, r))
        m = new(r[], S, cap, R, mcap)
        finalizer(x -> ccall((:slam_kfmap_destroy, LIB[]), Cint, (Ptr{Cvoid},), x.h), m)
    end
end
# sp: S x 32 stream parameters (Tcw, camera, distortion); acts on the streams k has selected
add_keyframe!(m::KeyframeMap, k::KeypointSet, sp::Matrix{Float64}) =
    (check(ccall((:slam_kfmap_add_keyframe, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), ctx(), m.h, k.h, sp)); m)
struct GatheredWindows
    n::Int; status::Vector{Int32}; win_stream::Vector{Int32}; Pn::Vector{Int32}; Mn::Vector{Int32}; On::Vector{Int32}
    θ::Vector{Float64}; θconst::Vector{UInt8}; pixels::Vector{Float64}; poses_ids::Vector{Int64}; points_ids::Vector{Int64}
    poses_remap::Vector{Int64}; points_remap::Vector{Int64}; obs_kf::Vector{Int64}; obs_kp::Vector{Int64}; obs_in_covmap::Vector{UInt8}
end
function gather(m::KeyframeMap, min_cov_score::Vector{Int32}; max_poses::Int = m.S * m.R, max_points::Int = m.S * min(m.mcap, 5 * m.cap), max_obs::Int = 8 * max_points)
    S = m.S
    g = GatheredWindows(0, zeros(Int32, S), zeros(Int32, S), zeros(Int32, S), zeros(Int32, S), zeros(Int32, S),
                        zeros(6 * max_poses + 3 * max_points), zeros(UInt8, max_poses), zeros(2 * max_obs), zeros(Int64, max_obs), zeros(Int64, max_obs),
                        zeros(Int64, max_poses), zeros(Int64, max_points), zeros(Int64, max_obs), zeros(Int64, max_obs), zeros(UInt8, max_obs))
    n = Ref{Int32}(0)
    GC.@preserve g min_cov_score begin
        w = KfmapWindows(S, max_poses, max_points, max_obs, pointer(g.status), pointer(g.win_stream), pointer(g.Pn), pointer(g.Mn), pointer(g.On),
                         pointer(g.θ), pointer(g.θconst), pointer(g.pixels), pointer(g.poses_ids), pointer(g.points_ids),
                         pointer(g.poses_remap), pointer(g.points_remap), pointer(g.obs_kf), pointer(g.obs_kp), pointer(g.obs_in_covmap))
        check(ccall((:slam_kfmap_ba_gather, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ref{KfmapWindows}, Ref{Int32}), ctx(), m.h, min_cov_score, w, n))
    end
    GatheredWindows(Int(n[]), g.status, g.win_stream, g.Pn, g.Mn, g.On, g.θ, g.θconst, g.pixels, g.poses_ids, g.points_ids,
                    g.poses_remap, g.points_remap, g.obs_kf, g.obs_kp, g.obs_in_covmap)
end
# θ / outliers: the arrays slam_local_ba_batch has written (windows back to back, in g.win_stream's order)
function update!(m::KeyframeMap, g::GatheredWindows, θ::Vector{Float64}, outliers::Vector{UInt8}; k::Union{Nothing, KeypointSet} = nothing)
    GC.@preserve g θ outliers check(ccall((:slam_kfmap_ba_update, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Float64}, Ptr{UInt8}),
        ctx(), m.h, k === nothing ? C_NULL : k.h, g.n, g.win_stream, θ, outliers))
    m
end
function download_keyframe(m::KeyframeMap, s::Integer, kfid::Integer)
    θ = zeros(6); ids = zeros(Int64, m.cap); upx = zeros(2, m.cap); live = zeros(UInt8, m.cap); n = Ref{Cint}(0)
    check(ccall((:slam_kfmap_download_keyframe, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}, Cint, Ref{Cint}),
                ctx(), m.h, s, kfid, θ, ids, upx, live, m.cap, n))
    n[] < 0 ? nothing : (θ = θ, ids = ids[1:n[]], upx = upx[:, 1:n[]], live = live[1:n[]] .!= 0)
end
function download_points(m::KeyframeMap, s::Integer)
    ids = zeros(Int64, m.mcap); xyz = zeros(3, m.mcap); flags = zeros(UInt8, m.mcap); off = zeros(Int32, m.mcap + 1); okf = zeros(Int32, m.mcap * m.R); n = Ref{Cint}(0)
    check(ccall((:slam_kfmap_download_points, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Cint, Cint, Ref{Cint}),
                ctx(), m.h, s, ids, xyz, flags, off, okf, m.mcap, m.mcap * m.R, n))
    (ids = ids[1:n[]], xyz = xyz[:, 1:n[]], flags = flags[1:n[]], observers = [okf[off[j] + 1:off[j + 1]] for j in 1:n[]])
end
reset!(m::KeyframeMap, s::Integer) = (check(ccall((:slam_kfmap_reset, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), ctx(), m.h, s)); m)
# map_filtering! (estimator.jl:358-406) for the streams of the last add_keyframe!: per-stream filtering_ratio and min_cov_score (S each); returns the S
# removed-masks (bit k % R per removed key-frame), or nothing with want_removed = false (enqueue-only).  newest(m): the streams' newest key-frame ids.
function filter_map!(m::KeyframeMap, filtering_ratio::Vector{Float64}, min_cov_score::Vector{Int32}; first_kfid::Integer = 20, want_removed::Bool = true)
    removed = zeros(UInt64, m.S)
    check(ccall((:slam_kfmap_filter, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Cint, Ptr{UInt64}),
                ctx(), m.h, filtering_ratio, min_cov_score, first_kfid, want_removed ? removed : C_NULL))
    want_removed ? removed : nothing
end
remove_keyframe!(m::KeyframeMap, s::Integer, kfid::Integer) =
    (check(ccall((:slam_kfmap_remove_keyframe, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint), ctx(), m.h, s, kfid)); m)
function newest(m::KeyframeMap)
    cur = zeros(Int32, m.S)
    check(ccall((:slam_kfmap_newest, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}), ctx(), m.h, cur))
    cur
end
# update_frame_covisibility! + match_local_map! (map_manager.jl:302-355, mapper.jl:265-383) on the map: enable_descriptors! once; per key-frame, after
# add_keyframe!, add_descriptors! with the device arrays slam_kpset_detect_describe filled (desc_dev: S x dcap x 4 UInt64, info_dev: S x 2 Int64), then
# local_map_match -> (status, n_pairs, pairs 2 x n (keypoint id, local-map id), dist), the streams back to back.  cam: 10 x S; lens distortion only after enable_pixels!.
enable_descriptors!(m::KeyframeMap, n_bits::Integer = 256) =
    (check(ccall((:slam_kfmap_enable_descriptors, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), ctx(), m.h, n_bits)); m)
add_descriptors!(m::KeyframeMap, desc_dev::Ptr{UInt64}, info_dev::Ptr{Int64}, dcap::Integer) =
    (check(ccall((:slam_kfmap_add_descriptors, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt64}, Ptr{Int64}, Cint), ctx(), m.h, desc_dev, info_dev, dcap)); m)
function local_map_match(m::KeyframeMap, cam::Matrix{Float64}, cell_size::Vector{Int32}, max_projection_distance::Vector{Float64},
                         max_descriptor_distance::Vector{Float64}; max_local::Integer = 10 * m.cap, cap_pairs::Integer = m.S * m.cap)
    status = zeros(Int32, m.S); n_pairs = zeros(Int32, m.S)
    pairs = zeros(Int64, 2, max(cap_pairs, 1)); dist = zeros(Float64, max(cap_pairs, 1))
    check(ccall((:slam_kfmap_local_map_match, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}, Cint),
                ctx(), m.h, cam, cell_size, max_projection_distance, max_descriptor_distance, max_local, status, n_pairs, pairs, dist, cap_pairs))
    n = sum(n_pairs)
    (status = status, n_pairs = n_pairs, pairs = pairs[:, 1:n], dist = dist[1:n])
end
# Raw pixels in the map (slam_kfmap_enable_pixels, before the first add_keyframe!): kp.pixel of every observation beside the undistorted one -- from
# then on local_map_match works on raw pixels, as find_best_match does, and takes cameras with lens distortion; merge! moves them with the
# observations.  keyframe_pixels: 2 x n raw pixels (y, x) of key-frame kfid of stream s (0-based s and kfid, as download_keyframe and every KeyframeMap
# wrapper) in download_keyframe's order, nothing when it is not in the ring.
enable_pixels!(m::KeyframeMap) =
    (check(ccall((:slam_kfmap_enable_pixels, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), m.h)); m)
function keyframe_pixels(m::KeyframeMap, s::Integer, kfid::Integer)
    px = zeros(2, m.cap); n = Ref{Cint}(0)
    check(ccall((:slam_kfmap_download_pixels, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Cint, Ref{Cint}),
                ctx(), m.h, s, kfid, px, m.cap, n))
    n[] < 0 ? nothing : px[:, 1:n[]]
end
# The local-map history (slam_kfmap_enable_local_map_history): frame.local_map_ids kept between key-frames -- from then on local_map_match follows the
# replace-or-union rule (map_manager.jl:350-354) and takes in the oldest covisible key-frame's set (mapper.jl:274-286).  local_map_ids: the set stored
# for key-frame kfid of stream s, ascending (an error where the ring does not hold the key-frame or no set was stored for it).
enable_local_map_history!(m::KeyframeMap) =
    (check(ccall((:slam_kfmap_enable_local_map_history, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx(), m.h)); m)
function local_map_ids(m::KeyframeMap, s::Integer, kfid::Integer)
    ids = zeros(Int64, m.mcap); n = Ref{Int32}(0)
    check(ccall((:slam_kfmap_download_local_map_ids, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Int64}, Cint, Ref{Int32}),
                ctx(), m.h, s, kfid, ids, m.mcap, n))
    ids[1:n[]]
end
# Descriptor rows (slam_kfmap_enable_descriptor_rows): a point keeps one row per key-frame, at most max_rows (2 .. 8) of them -- keyframes_descriptors
# (map_point.jl:15): a merge hands prev's rows to the surviving point, a removed observation takes its key-frame's row along, the match takes the minimum
# over all pairs of rows.  After enable_descriptors!; another max_rows on a second call is an error.  descriptor_rows: the rows of stream s's points in id
# order -- (ids, described, row_off (n + 1, 0-based), keys (key-frame ids, ascending per point), rows (4 x total), dropped).
enable_descriptor_rows!(m::KeyframeMap, max_rows::Integer = 4) =
    (check(ccall((:slam_kfmap_enable_descriptor_rows, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), ctx(), m.h, max_rows)); m)
function descriptor_rows(m::KeyframeMap, s::Integer; max_rows::Integer = 8)
    cap = m.mcap; ids = zeros(Int64, cap); described = zeros(UInt8, cap); off = zeros(Int32, cap + 1)
    keys = zeros(Int32, cap * max_rows); rows = zeros(UInt64, 4, cap * max_rows); n = Ref{Int32}(0); dropped = Ref{Int32}(0)
    check(ccall((:slam_kfmap_download_descriptor_rows, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt64}, Cint, Cint, Ref{Int32}, Ref{Int32}),
                ctx(), m.h, s, ids, described, off, keys, rows, cap, cap * max_rows, n, dropped))
    k = Int(n[]); r = Int(off[k + 1])
    (ids = ids[1:k], described = described[1:k] .!= 0, row_off = off[1:k + 1], keys = keys[1:r], rows = rows[:, 1:r], dropped = Int(dropped[]))
end
# merge_matches (mapper.jl:296-310) on the map: the pairs of the last local_map_match where they lie in HBM (n_pairs === nothing), or the caller's
# (n_pairs: S counts, pairs: 2 x n (prev id, new id), the streams back to back).  k: the KeypointSet whose live lists follow.  Returns the 4 x S counts
# (pairs applied, pairs skipped, observations renamed, status), or nothing with want_counts = false (enqueue-only).
function merge!(m::KeyframeMap, k::Union{Nothing, KeypointSet} = nothing; n_pairs::Union{Nothing, Vector{Int32}} = nothing,
                pairs::Union{Nothing, Matrix{Int64}} = nothing, want_counts::Bool = true)
    merged = zeros(Int32, 4, m.S)
    GC.@preserve n_pairs pairs merged check(ccall((:slam_kfmap_merge, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
        ctx(), m.h, k === nothing ? C_NULL : k.h, n_pairs === nothing ? Ptr{Int32}(C_NULL) : pointer(n_pairs),
        pairs === nothing ? Ptr{Int64}(C_NULL) : pointer(pairs), want_counts ? pointer(merged) : Ptr{Int32}(C_NULL)))
    want_counts ? merged : nothing
end
# triangulate_temporal! (mapper.jl:185-262) from the map's own key-frames, for the streams of the last add_keyframe! (call it right after): every 2-D
# point of the newest key-frame against its first observer as it is now, with the poses the last bundle adjustment left in the map.  cams: 4 x S
# (fx fy cx cy).  k: the KeypointSet whose lists take xyz and is_3d of the accepted points; a rejected keypoint STAYS in the list (triangulate_temporal!
# of the KeypointSet drops it).  Returns the 4 x S counts (candidates, triangulated, observations removed, skipped), or nothing with
# want_counts = false (enqueue-only).
function triangulate_temporal!(m::KeyframeMap, cams::Matrix{Float64}, k::Union{Nothing, KeypointSet} = nothing; max_error::Real = 3.0,
                               min_depth::Real = 0.1, min_parallax::Real = 20.0, want_counts::Bool = true)
    size(cams) == (4, m.S) || throw(ArgumentError("cams: 4 x S"))
    counts = zeros(Int32, 4, m.S)
    GC.@preserve cams counts check(ccall((:slam_kfmap_triangulate_temporal, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cdouble, Cdouble, Cdouble, Ptr{Int32}),
        ctx(), m.h, k === nothing ? C_NULL : k.h, pointer(cams), max_error, min_depth, min_parallax, want_counts ? pointer(counts) : Ptr{Int32}(C_NULL)))
    want_counts ? counts : nothing
end

# ---- one live stream, one call per frame (slam_frontend_*, include/slamhip.h): what run!()'s front-end task does per frame
# (front_end.jl:58-113, :454-470) and, at a key-frame, create_keyframe! + the mapper's stereo step (map_manager.jl:98-113, mapper.jl:51-66, :142-183),
# enqueued by ONE ccall; the keypoint list stays in HBM.  FrontEndConfig mirrors slam_frontend_config field for field (16 Int32, 9 Float64).
mutable struct FrontEndConfig
    H::Int32; W::Int32; pyramid_levels::Int32; pyramid_levels_3d::Int32; window::Int32; iterations::Int32
    max_points::Int32; radius::Int32; grid_rows::Int32; grid_cols::Int32; cell_size::Int32; cap::Int32
    pyr_mode::Int32; lookahead::Int32; right_target_only::Int32; reserved::Int32
    eig_thr::Float64; eps::Float64; max_distance::Float64; sigma_mask::Float64; min_response::Float64
    epipolar_error::Float64; max_error::Float64; min_depth::Float64; pyr_sigma::Float64
end
function FrontEndConfig(params, e; H::Integer, W::Integer, tolerance::Bool = false, lookahead::Bool = false)
    cells = e.grid_resolution[1] * e.grid_resolution[2]
    FrontEndConfig(H, W, params.pyramid_levels, 1, params.window_size, 30, e.max_points, e.radius, e.grid_resolution[1], e.grid_resolution[2], e.cell_size,
                   e.max_points + cells + 64, tolerance ? 3 : 1, lookahead ? 1 : 0, 1, 0,
                   1e-4, 1e-2, params.max_ktl_distance, 3.0, 1e-4, 2.0, params.max_reprojection_error, 0.1, params.pyramid_sigma)
end
struct LiveFrontEnd; h::Ptr{Cvoid}; cfg::FrontEndConfig; end
function LiveFrontEnd(cfg::FrontEndConfig; device::Integer = 0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:slam_frontend_create, LIB[]), Cint, (Cint, Ref{FrontEndConfig}, Ref{Ptr{Cvoid}}), device, cfg, r))
    LiveFrontEnd(r[], cfg)
end
close!(fe::LiveFrontEnd) = ccall((:slam_frontend_destroy, LIB[]), Cint, (Ptr{Cvoid},), fe.h)
# left / right: Matrix{UInt8} as the KITTI reader decodes them (column-major H x W); right === nothing unless the frame is a key-frame.  params /
# stereo_params: 32 Float64 each (stream_params of one stream); tri: 72 Float64 (P1, P2, T21, cam1, cam2, Twc).  Returns (frame index or -1, list length).
function step!(fe::LiveFrontEnd, left::Matrix{UInt8}, right::Union{Nothing, Matrix{UInt8}}, params::Vector{Float64}; prior::Integer = 1,
               stereo_params::Union{Nothing, Vector{Float64}} = nothing, stereo_prior::Integer = 2, tri::Union{Nothing, Vector{Float64}} = nothing)
    frame = Ref{Int32}(-1); n = Ref{Int32}(0)
    rc = GC.@preserve left right params stereo_params tri ccall((:slam_frontend_step, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Cint, Ptr{Float64}, Cint, Ptr{Float64}, Ptr{UInt8}, Ref{Int32}, Ref{Int32}),
        fe.h, left, right === nothing ? Ptr{UInt8}(C_NULL) : pointer(right), params, prior,
        stereo_params === nothing ? Ptr{Float64}(C_NULL) : pointer(stereo_params), stereo_prior, tri === nothing ? Ptr{Float64}(C_NULL) : pointer(tri), C_NULL, frame, n)
    rc == 0 || error("slam_frontend_step ($rc): ", unsafe_string(ccall((:slam_frontend_last_error, LIB[]), Cstring, (Ptr{Cvoid},), fe.h)))
    Int(frame[]), Int(n[])
end

end # module
