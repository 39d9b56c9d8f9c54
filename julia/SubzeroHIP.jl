# SubzeroHIP.jl -- Subzero.jl on an MI355X: the three per-timestep hot calls of `timestep_sim!`
# (src/simulation_components/simulation.jl:94-220) routed to libsubzero_hip.so through its C-ABI
# (include/subzero_hip.h).  Nothing in Subzero.jl is edited:
#
#     using Subzero, SubzeroHIP
#     sim = Simulation(...)                       # Float64 simulation, as usual
#     eng = SubzeroHIP.enable!(sim; device = 0)   # from here on the engine does the hot path
#     run!(sim)                                   # unchanged driver loop, unchanged output writers
#     SubzeroHIP.disable!()                       # back to the CPU path (and frees the device state)
#
# How it hooks in.  `timestep_sim!` calls
#     timestep_collisions!(floes, n_init_floes, domain, consts, Δt, collision_settings, spinlock)   collisions.jl:734
#     timestep_coupling!(model, Δt, consts, coupling_settings, floe_settings)                      coupling.jl:1705
#     timestep_floe_properties!(floes, tstep, Δt, floe_settings)                                   update_floe.jl:469
# whose reference methods leave the settings / constants arguments untyped.  This module adds methods that are MORE
# SPECIFIC in exactly those arguments (Float64 floes, `Constants{Float64}`, `CollisionSettings{Float64}`,
# `FloeSettings`), so Julia's dispatch picks them for every Float64 simulation once the module is loaded; each of them
# looks at `ENGINE[]` and either runs on the device or `invoke`s the reference method it shadows (no engine enabled:
# bit-for-bit the CPU behaviour).  The call sites in `timestep_sim!` do not change.
#
# Two ways to run:
#   * process mode (the three methods below): upload the floe columns, one device call, download what the reference
#     function would have mutated.  Works with every other process (fracture, ridging, welding, simplification, all
#     output writers), which keep seeing ordinary `StructArray{Floe}` state.
#   * resident mode (`run_resident!`): when no host-side process needs the floes between steps, whole batches of
#     `timestep_sim!` run with the state resident in HBM (`sz_step`); the batch ends early when a floe is tagged
#     remove / fuse, so that `simplify_floes!` runs at the step the reference would run it.
#
# NOT RUN in the build container (it has no Julia): the struct mirrors below are checked against the C header by
# tests/test_host_cpu.py::test_julia_struct_mirrors_match_the_header (field order, sizes and offsets), and the same
# call sequences are exercised on the GPU by the Python mirror of this file (subzero.jl_amd/host.py).
module SubzeroHIP

using Subzero
using StructArrays
import GeometryOps.GeoInterface as GI

export enable!, disable!, run_resident!, HIPEngine

const lib = get(ENV, "SUBZERO_HIP_LIB", "libsubzero_hip.so")

# ------------------------------------------------------------------------------------------------ C-ABI mirrors
# include/subzero_hip.h: sz_params
struct SzParams
    E::Float64
    nu::Float64
    mu::Float64
    rho_o::Float64
    rho_a::Float64
    Cd_io::Float64
    Cd_ia::Float64
    f::Float64
    turn_theta::Float64
    floe_floe_max_overlap::Float64
    floe_domain_max_overlap::Float64
    rho_i::Float64
    max_floe_height::Float64
    maximum_xi::Float64
    lambda::Float64
    coupling_dd::Int32
    _pad::Int32
end

# include/subzero_hip.h: sz_floe_columns (host pointers; C_NULL = column absent)
mutable struct SzFloeColumns
    cx::Ptr{Float64}
    cy::Ptr{Float64}
    rmax::Ptr{Float64}
    area::Ptr{Float64}
    height::Ptr{Float64}
    mass::Ptr{Float64}
    moment::Ptr{Float64}
    alpha::Ptr{Float64}
    u::Ptr{Float64}
    v::Ptr{Float64}
    xi::Ptr{Float64}
    p_dxdt::Ptr{Float64}
    p_dydt::Ptr{Float64}
    p_dalphadt::Ptr{Float64}
    p_dudt::Ptr{Float64}
    p_dvdt::Ptr{Float64}
    p_dxidt::Ptr{Float64}
    fxOA::Ptr{Float64}
    fyOA::Ptr{Float64}
    trqOA::Ptr{Float64}
    hflx_factor::Ptr{Float64}
    overarea::Ptr{Float64}
    coll_fx::Ptr{Float64}
    coll_fy::Ptr{Float64}
    coll_trq::Ptr{Float64}
    stress_accum::Ptr{Float64}
    stress_instant::Ptr{Float64}
    strain::Ptr{Float64}
    id::Ptr{Int64}
    ghost_id::Ptr{Int64}
    status::Ptr{Int32}
    vert_off::Ptr{Int32}
    vx::Ptr{Float64}
    vy::Ptr{Float64}
    sub_off::Ptr{Int32}
    sx::Ptr{Float64}
    sy::Ptr{Float64}
    ghost_off::Ptr{Int32}
    ghost_idx::Ptr{Int32}
end
SzFloeColumns() = SzFloeColumns(ntuple(_ -> C_NULL, 39)...)

# include/subzero_hip.h: sz_floe_columns_f32 -- the same columns of a Floe{Float32} host (the engine widens them on the way in and rounds
# them on the way out; see the Float32 section at the end of this file)
mutable struct SzFloeColumnsF32
    cx::Ptr{Float32}
    cy::Ptr{Float32}
    rmax::Ptr{Float32}
    area::Ptr{Float32}
    height::Ptr{Float32}
    mass::Ptr{Float32}
    moment::Ptr{Float32}
    alpha::Ptr{Float32}
    u::Ptr{Float32}
    v::Ptr{Float32}
    xi::Ptr{Float32}
    p_dxdt::Ptr{Float32}
    p_dydt::Ptr{Float32}
    p_dalphadt::Ptr{Float32}
    p_dudt::Ptr{Float32}
    p_dvdt::Ptr{Float32}
    p_dxidt::Ptr{Float32}
    fxOA::Ptr{Float32}
    fyOA::Ptr{Float32}
    trqOA::Ptr{Float32}
    hflx_factor::Ptr{Float32}
    overarea::Ptr{Float32}
    coll_fx::Ptr{Float32}
    coll_fy::Ptr{Float32}
    coll_trq::Ptr{Float32}
    stress_accum::Ptr{Float32}
    stress_instant::Ptr{Float32}
    strain::Ptr{Float32}
    id::Ptr{Int64}
    ghost_id::Ptr{Int64}
    status::Ptr{Int32}
    vert_off::Ptr{Int32}
    vx::Ptr{Float32}
    vy::Ptr{Float32}
    sub_off::Ptr{Int32}
    sx::Ptr{Float32}
    sy::Ptr{Float32}
    ghost_off::Ptr{Int32}
    ghost_idx::Ptr{Int32}
end
SzFloeColumnsF32() = SzFloeColumnsF32(ntuple(_ -> C_NULL, 39)...)

# include/subzero_hip.h: sz_stats
struct SzStats
    M::Int64
    N::Int64
    n_ring_points::Int64
    n_sub_points::Int64
    n_pairs::Int64
    n_pair_ring_points::Int64
    n_pair_rows::Int64
    n_elem_items::Int64
    n_elem_rows::Int64
    n_inter_rows::Int64
    n_ghosts::Int64
    warn_height::Int64
    warn_force::Int64
    warn_vel::Int64
    warn_xi::Int64
    n_trace_fail::Int64
    n_halo::Int64
    n_pairs_clipped::Int64
    n_status_remove::Int64
    n_status_fuse::Int64
    n_retry::Int64
    acc_narrow_launches::Int64
    acc_pair_items::Int64
    acc_pair_ring_points::Int64
    acc_pair_rows::Int64
    acc_elem_items::Int64
    acc_elem_rows::Int64
    acc_dir_checks::Int64
    acc_dir_checks_certified::Int64
end

const SZ_COLLISIONS_ON = Int32(1)
const SZ_COUPLING_ON = Int32(2)
const SZ_NO_STOP = Int32(4)
const SZ_FRAC_OFF = Int32(0)
const SZ_FRAC_HIBLER = Int32(1)
const SZ_FRAC_POLYGON = Int32(2)
boundary_kind(::OpenBoundary) = Int32(0)
boundary_kind(::PeriodicBoundary) = Int32(1)
boundary_kind(::CollisionBoundary) = Int32(2)
boundary_kind(::MovingBoundary) = Int32(3)

# ------------------------------------------------------------------------------------------------ the engine
mutable struct HIPEngine
    ctx::Ptr{Cvoid}
    two_way::Bool
    Nx::Int
    Ny::Int
    max_vertices::Int32          # SimplificationSettings / FloeSettings values of the simulation the engine was made for
    min_floe_area::Float64       # (sz_simplify_check)
    min_floe_height::Float64
    host_rows::Vector{Int}       # per host row the row it had at the last upload! (the device removes floes: origin, pull_state!)
    rec_floe::Vector{Tuple{Int, UInt64}}   # device floe writer k + 1 -> (index in sim.writers.floewriters, its column mask); set_floe_output!
                                           # (the lists a writer records follow from its outputs: frame_lists)
    rec_grid::Vector{Int}        # device grid writer k + 1 -> index in sim.writers.gridwriters; set_grid_output!
end

const ENGINE = Ref{Union{Nothing, HIPEngine}}(nothing)

last_error(eng) = unsafe_string(@ccall lib.sz_last_error(eng.ctx::Ptr{Cvoid})::Cstring)
function check(eng::HIPEngine, rc::Integer)
    rc == 0 || error("libsubzero_hip: error $rc: $(last_error(eng))")
    return
end

# lattice fields are (Nx+1) x (Ny+1) column-major in Julia; the library wants element [ix][iy] at ix*(Ny+1)+iy
lattice(m::AbstractMatrix) = collect(Float64, permutedims(m))
unlattice(buf::Vector{Float64}, Nx, Ny) = permutedims(reshape(buf, Ny + 1, Nx + 1))

"""
    enable!(sim; device = 0) -> HIPEngine

Create the device context for `sim` (constants, settings, domain, topography, ocean / atmosphere lattices) and route
the hot calls of every Float64 simulation to it until `disable!()`.
"""
function enable!(sim; device::Integer = 0)
    disable!()
    ctx = @ccall lib.sz_create(device::Cint)::Ptr{Cvoid}
    ctx == C_NULL && error("sz_create: no HIP device (the engine has no CPU fallback)")
    model, c, cs, fs, cp = sim.model, sim.consts, sim.collision_settings, sim.floe_settings, sim.coupling_settings
    grid = model.grid
    eng = HIPEngine(ctx, cp.two_way_coupling_on, grid.Nx, grid.Ny, Int32(sim.simp_settings.max_vertices),
                    Float64(fs.min_floe_area), Float64(fs.min_floe_height), Int[], Tuple{Int, UInt64}[], Int[])
    λ = hasproperty(fs.stress_calculator, :λ) ? Float64(fs.stress_calculator.λ) :
        error("SubzeroHIP implements DecayAreaScaledCalculator (stress_calculators.jl:82) only")
    p = Ref(SzParams(c.E, c.ν, c.μ, c.ρo, c.ρa, c.Cd_io, c.Cd_ia, c.f, c.turnθ, cs.floe_floe_max_overlap,
                     cs.floe_domain_max_overlap, fs.ρi, fs.max_floe_height, fs.maximum_ξ, λ, Int32(cp.Δd), Int32(0)))
    check(eng, @ccall lib.sz_set_params(ctx::Ptr{Cvoid}, p::Ptr{SzParams})::Cint)
    push_domain!(eng, model.domain)
    push_fields!(eng, model)
    if cp.two_way_coupling_on
        check(eng, @ccall lib.sz_set_two_way(ctx::Ptr{Cvoid}, 1::Int32, c.Cd_ao::Float64, c.k::Float64, c.L::Float64,
                                             sim.Δt::Int32)::Cint)
        to, ta = lattice(model.ocean.temp), lattice(model.atmos.temp)
        check(eng, @ccall lib.sz_set_temps(ctx::Ptr{Cvoid}, to::Ptr{Float64}, ta::Ptr{Float64})::Cint)
    end
    ENGINE[] = eng
    return eng
end

function disable!()
    eng = ENGINE[]
    if eng !== nothing
        @ccall lib.sz_destroy(eng.ctx::Ptr{Cvoid})::Cvoid
        ENGINE[] = nothing
    end
    return
end

function push_domain!(eng::HIPEngine, domain)
    bnds = (domain.north, domain.south, domain.east, domain.west)
    kinds = Int32[boundary_kind(b) for b in bnds]
    vals = Float64[b.val for b in bnds]
    rects = Float64[]
    for b in bnds
        (x0, xf), (y0, yf) = GI.extent(b.poly)
        append!(rects, (x0, xf, y0, yf))
    end
    bu = Float64[b isa MovingBoundary ? b.u : 0.0 for b in bnds]
    bv = Float64[b isa MovingBoundary ? b.v : 0.0 for b in bnds]
    check(eng, @ccall lib.sz_set_domain(eng.ctx::Ptr{Cvoid}, kinds::Ptr{Int32}, vals::Ptr{Float64}, rects::Ptr{Float64},
                                        bu::Ptr{Float64}, bv::Ptr{Float64})::Cint)
    topo = domain.topography
    nt = length(topo)
    off = Int32[0]; tx = Float64[]; ty = Float64[]
    for i in 1:nt
        for pt in GI.getpoint(GI.getexterior(topo.poly[i]))
            push!(tx, GI.x(pt)); push!(ty, GI.y(pt))
        end
        push!(off, Int32(length(tx)))
    end
    tcx = Float64[topo.centroid[i][1] for i in 1:nt]; tcy = Float64[topo.centroid[i][2] for i in 1:nt]
    trm = Float64[topo.rmax[i] for i in 1:nt]
    check(eng, @ccall lib.sz_set_topography(eng.ctx::Ptr{Cvoid}, nt::Int32, off::Ptr{Int32}, tx::Ptr{Float64}, ty::Ptr{Float64},
                                            tcx::Ptr{Float64}, tcy::Ptr{Float64}, trm::Ptr{Float64})::Cint)
    return
end

function push_fields!(eng::HIPEngine, model)
    g, o, a = model.grid, model.ocean, model.atmos
    uo, vo, hf, ua, va = lattice(o.u), lattice(o.v), lattice(o.hflx_factor), lattice(a.u), lattice(a.v)
    check(eng, @ccall lib.sz_set_fields(eng.ctx::Ptr{Cvoid}, g.Nx::Int32, g.Ny::Int32, g.x0::Float64, g.xf::Float64,
                                        g.y0::Float64, g.yf::Float64, uo::Ptr{Float64}, vo::Ptr{Float64}, hf::Ptr{Float64},
                                        ua::Ptr{Float64}, va::Ptr{Float64})::Cint)
    return
end

# ------------------------------------------------------------------------------------------------ pack / unpack
# Everything the pointers of an SzFloeColumns point into (kept alive by the caller with GC.@preserve).
struct Packed
    cols::SzFloeColumns
    cx::Vector{Float64}; cy::Vector{Float64}
    coll_fx::Vector{Float64}; coll_fy::Vector{Float64}
    sa::Vector{Float64}; si::Vector{Float64}; strain::Vector{Float64}
    status::Vector{Int32}
    vert_off::Vector{Int32}; vx::Vector{Float64}; vy::Vector{Float64}
    sub_off::Vector{Int32}; sx::Vector{Float64}; sy::Vector{Float64}
    ghost_off::Vector{Int32}; ghost_idx::Vector{Int32}
    id::Vector{Int64}; ghost_id::Vector{Int64}
end

tensor4(m) = (m[1, 1], m[1, 2], m[2, 1], m[2, 2])     # 2x2 -> the library's order 11, 12, 21, 22

"""
    pack(floes, n_parents) -> Packed

The hot columns of `StructArray{Floe{Float64}}` (floe.jl:24-77) as `sz_floe_columns`: scalar columns are passed where
they lie (they are contiguous `Vector{Float64}` / `Vector{Int}` already), ragged ones are flattened to CSR.
"""
function pack(floes::StructArray{<:Floe{Float64}}, n_parents::Integer)
    M = length(floes)
    cx = Float64[c[1] for c in floes.centroid]; cy = Float64[c[2] for c in floes.centroid]
    coll_fx = Float64[f[1, 1] for f in floes.collision_force]; coll_fy = Float64[f[1, 2] for f in floes.collision_force]
    sa = Vector{Float64}(undef, 4M); si = similar(sa); st = similar(sa)
    for i in 1:M
        sa[4i-3:4i] .= tensor4(floes.stress_accum[i]); si[4i-3:4i] .= tensor4(floes.stress_instant[i])
        st[4i-3:4i] .= tensor4(floes.strain[i])
    end
    status = Int32[Int32(s.tag) for s in floes.status]            # active = 1, remove = 2, fuse = 3 (floe.jl:8-12)
    vert_off = Vector{Int32}(undef, M + 1); vert_off[1] = 0
    vx = Float64[]; vy = Float64[]
    for i in 1:M                                                   # the exterior ring, closed (floe_utils.jl:10-17)
        for pt in GI.getpoint(GI.getexterior(floes.poly[i]))
            push!(vx, GI.x(pt)); push!(vy, GI.y(pt))
        end
        vert_off[i+1] = length(vx)
    end
    sub_off = Vector{Int32}(undef, n_parents + 1); sub_off[1] = 0
    sx = Float64[]; sy = Float64[]
    for i in 1:n_parents
        append!(sx, floes.x_subfloe_points[i]); append!(sy, floes.y_subfloe_points[i])
        sub_off[i+1] = length(sx)
    end
    ghost_off = Vector{Int32}(undef, M + 1); ghost_off[1] = 0
    ghost_idx = Int32[]
    for i in 1:M
        append!(ghost_idx, Int32.(floes.ghosts[i] .- 1))           # 0-based in the C-ABI
        ghost_off[i+1] = length(ghost_idx)
    end
    id = Vector{Int64}(floes.id); ghost_id = Vector{Int64}(floes.ghost_id)
    c = SzFloeColumns()
    c.cx = pointer(cx); c.cy = pointer(cy)
    c.rmax = pointer(floes.rmax); c.area = pointer(floes.area); c.height = pointer(floes.height)
    c.mass = pointer(floes.mass); c.moment = pointer(floes.moment); c.alpha = pointer(floes.α)
    c.u = pointer(floes.u); c.v = pointer(floes.v); c.xi = pointer(floes.ξ)
    c.p_dxdt = pointer(floes.p_dxdt); c.p_dydt = pointer(floes.p_dydt); c.p_dalphadt = pointer(floes.p_dαdt)
    c.p_dudt = pointer(floes.p_dudt); c.p_dvdt = pointer(floes.p_dvdt); c.p_dxidt = pointer(floes.p_dξdt)
    c.fxOA = pointer(floes.fxOA); c.fyOA = pointer(floes.fyOA); c.trqOA = pointer(floes.trqOA)
    c.hflx_factor = pointer(floes.hflx_factor); c.overarea = pointer(floes.overarea)
    c.coll_fx = pointer(coll_fx); c.coll_fy = pointer(coll_fy); c.coll_trq = pointer(floes.collision_trq)
    c.stress_accum = pointer(sa); c.stress_instant = pointer(si); c.strain = pointer(st)
    c.id = pointer(id); c.ghost_id = pointer(ghost_id); c.status = pointer(status)
    c.vert_off = pointer(vert_off); c.vx = pointer(vx); c.vy = pointer(vy)
    c.sub_off = pointer(sub_off); c.sx = pointer(sx); c.sy = pointer(sy)
    if M > n_parents
        c.ghost_off = pointer(ghost_off); c.ghost_idx = pointer(ghost_idx)
    end
    return Packed(c, cx, cy, coll_fx, coll_fy, sa, si, st, status, vert_off, vx, vy, sub_off, sx, sy, ghost_off, ghost_idx,
                  id, ghost_id)
end

function upload!(eng::HIPEngine, floes, n_parents)
    P = pack(floes, n_parents)
    GC.@preserve P floes begin
        check(eng, @ccall lib.sz_upload_floes(eng.ctx::Ptr{Cvoid}, length(floes)::Int64, n_parents::Int64,
                                              P.cols::Ref{SzFloeColumns})::Cint)
    end
    eng.host_rows = collect(1:length(floes))
    return P
end

# floe.interactions of every floe -> the device (calc_stress!, update_floe.jl:392-414, reads them)
function upload_interactions!(eng::HIPEngine, floes)
    M = length(floes)
    off = Vector{Int32}(undef, M + 1); off[1] = 0
    for i in 1:M
        off[i+1] = off[i] + floes.num_inters[i]
    end
    rows = Matrix{Float64}(undef, 7, max(Int(off[end]), 1))          # row-major k x 7 on the C side
    for i in 1:M, k in 1:floes.num_inters[i]
        rows[:, off[i]+k] .= @view floes.interactions[i][k, :]
    end
    check(eng, @ccall lib.sz_upload_interactions(eng.ctx::Ptr{Cvoid}, off::Ptr{Int32}, rows::Ptr{Float64})::Cint)
    return
end

function stats(eng::HIPEngine)
    st = Ref{SzStats}()
    check(eng, @ccall lib.sz_get_stats(eng.ctx::Ptr{Cvoid}, st::Ptr{SzStats})::Cint)
    return st[]
end

# scalar columns come back where they lie; `P` holds the flattened ones
function download!(eng::HIPEngine, floes, P::Packed)
    GC.@preserve P floes begin
        check(eng, @ccall lib.sz_download_floes(eng.ctx::Ptr{Cvoid}, P.cols::Ref{SzFloeColumns})::Cint)
    end
    return
end

function unpack_status!(floes, P::Packed)
    for i in eachindex(floes)
        floes.status[i].tag = Subzero.StatusTag(P.status[i])
    end
end

# ------------------------------------------------------------------------------------------------ the three hot calls
# timestep_collisions! (collisions.jl:734-864): what it mutates is reproduced on the host -- interactions (k x 7, floeidx
# column as the reference stores it), num_inters, overarea, status (+ fuse_idx), collision_force / collision_trq of the
# parents, MovingBoundary walls.
function Subzero.timestep_collisions!(floes::StructArray{<:Floe{Float64}}, n_init_floes, domain::Domain,
                                      consts::Constants{Float64}, Δt, collision_settings::CollisionSettings{Float64}, spinlock)
    eng = ENGINE[]
    if eng === nothing
        return invoke(Subzero.timestep_collisions!, Tuple{StructArray{<:Floe{Float64}}, Any, Any, Any, Any, Any, Any},
                      floes, n_init_floes, domain, consts, Δt, collision_settings, spinlock)
    end
    M = length(floes)
    P = upload!(eng, floes, n_init_floes)           # Julia's add_ghosts! has run: ghost rows and links go up as they are
    check(eng, @ccall lib.sz_timestep_collisions(eng.ctx::Ptr{Cvoid}, n_init_floes::Int64, Δt::Int32)::Cint)
    st = stats(eng)
    off = Vector{Int32}(undef, M + 1); rows = Matrix{Float64}(undef, 7, max(Int(st.n_inter_rows), 1))
    check(eng, @ccall lib.sz_download_interactions(eng.ctx::Ptr{Cvoid}, off::Ptr{Int32}, rows::Ptr{Float64})::Cint)
    download!(eng, floes, P)                        # overarea, collision_trq in place; coll_fx / coll_fy / status in P
    for i in 1:M
        r = off[i]+1:off[i+1]
        floes.interactions[i] = permutedims(rows[:, r])            # k x 7: floeidx xforce yforce xpoint ypoint torque overlap
        floes.num_inters[i] = length(r)
        floes.collision_force[i][1, 1] = P.coll_fx[i]; floes.collision_force[i][1, 2] = P.coll_fy[i]
    end
    unpack_status!(floes, P)
    foff = Vector{Int32}(undef, M + 1)
    check(eng, @ccall lib.sz_download_fuse(eng.ctx::Ptr{Cvoid}, foff::Ptr{Int32}, C_NULL::Ptr{Int32})::Cint)
    fidx = Vector{Int32}(undef, max(Int(foff[end]), 1))
    check(eng, @ccall lib.sz_download_fuse(eng.ctx::Ptr{Cvoid}, foff::Ptr{Int32}, fidx::Ptr{Int32})::Cint)
    for i in 1:M
        empty!(floes.status[i].fuse_idx)
        append!(floes.status[i].fuse_idx, Int.(fidx[foff[i]+1:foff[i+1]]) .+ 1)
    end
    pull_moving_boundaries!(eng, domain)
    return
end

# MovingBoundary walls moved on the device (update_boundaries!, collisions.jl:565-571): val and poly back to the host
function pull_moving_boundaries!(eng::HIPEngine, domain)
    bnds = (domain.north, domain.south, domain.east, domain.west)
    any(b -> b isa MovingBoundary, bnds) || return
    vals = Vector{Float64}(undef, 4); rects = Vector{Float64}(undef, 16)
    check(eng, @ccall lib.sz_get_boundary_vals(eng.ctx::Ptr{Cvoid}, vals::Ptr{Float64})::Cint)
    check(eng, @ccall lib.sz_get_boundary_rects(eng.ctx::Ptr{Cvoid}, rects::Ptr{Float64})::Cint)
    for (k, b) in enumerate(bnds)
        b isa MovingBoundary || continue
        b.val = vals[k]
        x0, xf, y0, yf = rects[4k-3:4k]
        b.poly = Subzero._make_bounding_box_polygon(Float64, x0, xf, y0, yf)
    end
    return
end

# timestep_coupling! (coupling.jl:1705-1738): fxOA, fyOA, trqOA, hflx_factor, status (remove: no sub-floe point in
# bounds); with two-way coupling the ice-on-ocean stress fields.  grid.floe_locations / ocean.scells are bookkeeping of
# the CPU algorithm and are not materialised (only calc_two_way_coupling!, replaced here, reads them).
function Subzero.timestep_coupling!(model::Model{Float64}, Δt, consts::Constants{Float64},
                                    coupling_settings::CouplingSettings, floe_settings::FloeSettings)
    eng = ENGINE[]
    if eng === nothing
        return invoke(Subzero.timestep_coupling!, Tuple{Any, Any, Any, Any, Any}, model, Δt, consts, coupling_settings,
                      floe_settings)
    end
    floes = model.floes
    P = upload!(eng, floes, length(floes))
    check(eng, @ccall lib.sz_timestep_coupling(eng.ctx::Ptr{Cvoid})::Cint)
    download!(eng, floes, P)
    unpack_status!(floes, P)
    coupling_settings.two_way_coupling_on && pull_ocean_stress!(eng, model.ocean)
    return
end

function pull_ocean_stress!(eng::HIPEngine, ocean)
    n = (eng.Nx + 1) * (eng.Ny + 1)
    tx, ty, sf, hf = (Vector{Float64}(undef, n) for _ in 1:4)
    check(eng, @ccall lib.sz_download_ocean_stress(eng.ctx::Ptr{Cvoid}, tx::Ptr{Float64}, ty::Ptr{Float64}, sf::Ptr{Float64},
                                                   hf::Ptr{Float64})::Cint)
    ocean.τx .= unlattice(tx, eng.Nx, eng.Ny); ocean.τy .= unlattice(ty, eng.Nx, eng.Ny)
    ocean.si_frac .= unlattice(sf, eng.Nx, eng.Ny); ocean.hflx_factor .= unlattice(hf, eng.Nx, eng.Ny)
    return
end

# timestep_floe_properties! (update_floe.jl:469-551): stress, guards, AB2 update, ring move, strain.  calc_stress! reads
# floe.interactions, which other host processes may have touched since the collisions: they go up with the columns.
function Subzero.timestep_floe_properties!(floes::StructArray{<:Floe{Float64}}, tstep, Δt, floe_settings::FloeSettings)
    eng = ENGINE[]
    if eng === nothing
        return invoke(Subzero.timestep_floe_properties!, Tuple{StructArray{<:Floe{Float64}}, Any, Any, Any}, floes, tstep, Δt,
                      floe_settings)
    end
    P = upload!(eng, floes, length(floes))
    upload_interactions!(eng, floes)
    check(eng, @ccall lib.sz_timestep_floe_properties(eng.ctx::Ptr{Cvoid}, Δt::Int32)::Cint)
    download!(eng, floes, P)
    unpack_geometry!(floes, P)
    return
end

# centroid, poly / coords and the three 2 x 2 tensors back into the per-floe objects
function unpack_geometry!(floes, P::Packed)
    for i in eachindex(floes)
        floes.centroid[i][1] = P.cx[i]; floes.centroid[i][2] = P.cy[i]
        r = P.vert_off[i]+1:P.vert_off[i+1]
        ring = [[P.vx[k], P.vy[k]] for k in r]
        floes.coords[i] = [ring]
        floes.poly[i] = Subzero.make_polygon(floes.coords[i])
        for (m, src) in ((floes.stress_accum[i], P.sa), (floes.stress_instant[i], P.si), (floes.strain[i], P.strain))
            m[1, 1], m[1, 2], m[2, 1], m[2, 2] = src[4i-3], src[4i-2], src[4i-1], src[4i]
        end
    end
    return
end

# ------------------------------------------------------------------------------------------------ fracture criteria
"""
    set_fracture!(eng, sim)

The simulation's fracture criterion on the device (`sz_set_fracture`): `FractureSettings.Δt`, a `HiblerYieldCurve` (rebuilt from the
mean floe height on every fracture step, `update_criteria!`) or a `MohrsCone` (its fixed polygon), `FloeSettings.min_floe_area` and
`DecayAreaScaledCalculator.α`.  Fractures off: `SZ_FRAC_OFF`.
"""
function set_fracture!(eng::HIPEngine, sim)
    fs = sim.fracture_settings
    if !fs.fractures_on
        check(eng, @ccall lib.sz_set_fracture(eng.ctx::Ptr{Cvoid}, SZ_FRAC_OFF::Int32, Int32(1)::Int32, 0.0::Float64, 0.0::Float64,
                                              Int32(0)::Int32, C_NULL::Ptr{Float64}, C_NULL::Ptr{Float64}, 0.0::Float64, 1.0::Float64)::Cint)
        return
    end
    sc = sim.floe_settings.stress_calculator
    sc isa Subzero.DecayAreaScaledCalculator ||
        error("run_resident!: fractures need a DecayAreaScaledCalculator stress calculator (got $(typeof(sc)))")
    α, amin, crit = Float64(sc.α), Float64(sim.floe_settings.min_floe_area), fs.criteria
    if crit isa Subzero.HiblerYieldCurve
        check(eng, @ccall lib.sz_set_fracture(eng.ctx::Ptr{Cvoid}, SZ_FRAC_HIBLER::Int32, Int32(fs.Δt)::Int32, Float64(crit.pstar)::Float64,
                                              Float64(crit.c)::Float64, Int32(0)::Int32, C_NULL::Ptr{Float64}, C_NULL::Ptr{Float64},
                                              α::Float64, amin::Float64)::Cint)
    elseif crit isa Subzero.MohrsCone
        ring = Subzero.find_poly_coords(crit.poly)[1]
        px, py = Float64[Float64(q[1]) for q in ring], Float64[Float64(q[2]) for q in ring]
        check(eng, @ccall lib.sz_set_fracture(eng.ctx::Ptr{Cvoid}, SZ_FRAC_POLYGON::Int32, Int32(fs.Δt)::Int32, 0.0::Float64, 0.0::Float64,
                                              Int32(length(px))::Int32, px::Ptr{Float64}, py::Ptr{Float64}, α::Float64, amin::Float64)::Cint)
    else
        error("run_resident!: fracture criterion $(typeof(crit)) has no device form (HiblerYieldCurve, MohrsCone)")
    end
    return
end

# determine_fractures on the resident state: how many floes would fracture now
function fracture_candidates(eng::HIPEngine)
    n = Ref{Int32}(0)
    check(eng, @ccall lib.sz_fracture_candidates(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, C_NULL::Ptr{Int32})::Cint)
    return Int(n[])
end

# ------------------------------------------------------------------------------------------------ welding
"""
    set_welding!(eng, sim)

The simulation's `WeldSettings` on the device (`sz_set_welding`): `Δts`, `Nxs`, `Nys` in the order the settings keep them (sorted by `Δt`,
largest first) and `max_weld_area`.  Welding off: no sets.
"""
function set_welding!(eng::HIPEngine, sim)
    ws = sim.weld_settings
    if !ws.weld_on
        check(eng, @ccall lib.sz_set_welding(eng.ctx::Ptr{Cvoid}, Int32(0)::Int32, C_NULL::Ptr{Int32}, C_NULL::Ptr{Int32}, C_NULL::Ptr{Int32},
                                             1.0::Float64)::Cint)
        return
    end
    dts, nxs, nys = Int32.(ws.Δts), Int32.(ws.Nxs), Int32.(ws.Nys)
    check(eng, @ccall lib.sz_set_welding(eng.ctx::Ptr{Cvoid}, Int32(length(dts))::Int32, dts::Ptr{Int32}, nxs::Ptr{Int32}, nys::Ptr{Int32},
                                         Float64(ws.max_weld_area)::Float64)::Cint)
    return
end

"""
    weld_overlaps(eng, nx, ny, max_weld_area) -> (i, j, inter_area)

The welding overlap table of the resident state (`sz_weld_overlaps`): the pairs `i < j` (1-based) `timestep_welding!` would clip for an
`nx` x `ny` welding grid and find overlapping, with their intersection areas, in the order its loops visit them (bin, then `i`, then `j`).
"""
function weld_overlaps(eng::HIPEngine, nx::Integer, ny::Integer, max_weld_area::Real)
    n = Ref{Int32}(0)
    check(eng, @ccall lib.sz_weld_overlaps(eng.ctx::Ptr{Cvoid}, Int32(nx)::Int32, Int32(ny)::Int32, Float64(max_weld_area)::Float64, n::Ptr{Int32},
                                           Int32(0)::Int32, C_NULL::Ptr{Int32}, C_NULL::Ptr{Int32}, C_NULL::Ptr{Float64})::Cint)
    cap = max(Int(n[]), 1)
    ti, tj, ta = Vector{Int32}(undef, cap), Vector{Int32}(undef, cap), Vector{Float64}(undef, cap)
    check(eng, @ccall lib.sz_weld_overlaps(eng.ctx::Ptr{Cvoid}, Int32(nx)::Int32, Int32(ny)::Int32, Float64(max_weld_area)::Float64, n::Ptr{Int32},
                                           Int32(cap)::Int32, ti::Ptr{Int32}, tj::Ptr{Int32}, ta::Ptr{Float64})::Cint)
    m = Int(n[])
    return (i = Int.(ti[1:m]) .+ 1, j = Int.(tj[1:m]) .+ 1, inter_area = ta[1:m])
end

"""
    timestep_welding!(floes, max_floe_id, table, weld_settings, floe_settings, weld_idx, Δt, rng)

`Subzero.timestep_welding!` (welding.jl:91-182) with the clip of every candidate pair replaced by a lookup in the device's overlap `table`
(`weld_overlaps` for the `Nxs[weld_idx]` x `Nys[weld_idx]` grid, taken from the state the call starts from).  The table lists exactly the pairs
with `inter_area > 0` in the order the reference's loops reach them, grouped by bin and by `i`; a pair that is not listed has `inter_area = 0`,
for which the reference draws no random number and welds nothing.  Every entry is looked at when its turn comes: both floes still active and
under `max_weld_area`, one draw per entry, the union-area window; the partners of one `i` are then fused largest overlap first until the welded
floe would exceed `max_weld_area`.  The areas in the table stay valid through the call: floe `i` changes shape only after its own entries have been
read, and a `j` that was fused away earlier is tagged `remove` and skipped.
"""
function timestep_welding!(floes, max_floe_id, table, weld_settings, floe_settings, weld_idx, Δt, rng = Subzero.Xoshiro())
    ws = weld_settings
    nent = length(table.i)
    e = 1
    while e <= nent
        i = table.i[e]
        stop = e
        while stop < nent && table.i[stop+1] == i
            stop += 1
        end
        partners = Tuple{Int, Float64}[]
        if floes.status[i].tag == Subzero.active && floes.area[i] < ws.max_weld_area
            for q in e:stop
                j, a = table.j[q], table.inter_area[q]
                (floes.status[j].tag == Subzero.active && floes.area[j] < ws.max_weld_area) || continue
                prob = ws.welding_coeff * (a / floes.area[i])
                union_area = floes.area[i] + floes.area[j] - a
                if a > 0 && prob > rand(rng) && ws.min_weld_area < union_area && ws.max_weld_area > union_area
                    push!(partners, (j, a))
                end
            end
        end
        sort!(partners, by = last, rev = true)
        for (j, a) in partners
            floes.area[i] + floes.area[j] - a > ws.max_weld_area && break
            Subzero.fuse_two_floes!(Subzero.get_floe(floes, i), Subzero.get_floe(floes, j), Δt, floe_settings, max_floe_id, rng)
            floes.id[i] = -1          # numbered below, in index order, as the reference does
        end
        e = stop + 1
    end
    for i in eachindex(floes.id)
        if floes.id[i] == -1
            max_floe_id += 1
            floes.id[i] = max_floe_id
        end
    end
    return max_floe_id
end

# ------------------------------------------------------------------------------------------------ removal and dissolution
"""
    set_removal!(eng, sim)

`remove_floes!` (simplification.jl:279-314) on the device (`sz_set_removal`): `SimplificationSettings.max_vertices` (`typemax(Int32)` with
`smooth_vertices_on == false`: no ring is then smoothed) and `FloeSettings.min_floe_area` / `min_floe_height`.  A batch of `sz_step` then goes
on past a step that tagged a floe `remove`, unless that step needs the host (a `fuse` tag, a ring to smooth, a fracture candidate, a welding step).
"""
function set_removal!(eng::HIPEngine, sim)
    maxv = sim.simp_settings.smooth_vertices_on ? Int32(min(sim.simp_settings.max_vertices, typemax(Int32))) : typemax(Int32)
    check(eng, @ccall lib.sz_set_removal(eng.ctx::Ptr{Cvoid}, Int32(1)::Int32, maxv::Int32, eng.min_floe_area::Float64,
                                         eng.min_floe_height::Float64)::Cint)
    return
end

"""
    remove_floes!(eng) -> (done, n_removed, n_dissolved)

One pass of `remove_floes!` on the resident state (`sz_remove_floes`).  `done == false`: the pass was declined and nothing changed --
`simplify_floes!` has more to do than removing, and runs on the host.
"""
function remove_floes!(eng::HIPEngine)
    done, nr, nd = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    check(eng, @ccall lib.sz_remove_floes(eng.ctx::Ptr{Cvoid}, done::Ptr{Int32}, nr::Ptr{Int32}, nd::Ptr{Int32})::Cint)
    return (done = done[] != 0, n_removed = Int(nr[]), n_dissolved = Int(nd[]))
end

# per resident parent the (1-based) row it had at the last upload!
function origin(eng::HIPEngine)
    n = Int(stats(eng).N)
    o = Vector{Int32}(undef, max(n, 1))
    check(eng, @ccall lib.sz_download_origin(eng.ctx::Ptr{Cvoid}, o::Ptr{Int32})::Cint)
    return Int.(o[1:n]) .+ 1
end

# ocean.dissolved: the host's matrix to the device, and the device's running lattice back over it
function push_dissolved!(eng::HIPEngine, ocean)
    d = lattice(ocean.dissolved)
    check(eng, @ccall lib.sz_upload_dissolved(eng.ctx::Ptr{Cvoid}, d::Ptr{Float64})::Cint)
    return
end
function pull_dissolved!(eng::HIPEngine, ocean)
    d = Vector{Float64}(undef, (eng.Nx + 1) * (eng.Ny + 1))
    check(eng, @ccall lib.sz_download_dissolved(eng.ctx::Ptr{Cvoid}, d::Ptr{Float64})::Cint)
    ocean.dissolved .= unlattice(d, eng.Nx, eng.Ny)
    return
end

# ------------------------------------------------------------------------------------------------ rows down, rows back
# floe.interactions of the floes of a list as the CSR pair the C side takes (row-major k x 7)
function interactions_csr(floes)
    M = length(floes)
    off = Vector{Int32}(undef, M + 1); off[1] = 0
    for i in 1:M
        off[i+1] = off[i] + floes.num_inters[i]
    end
    rows = Matrix{Float64}(undef, 7, max(Int(off[end]), 1))
    for i in 1:M, k in 1:floes.num_inters[i]
        rows[:, off[i]+k] .= @view floes.interactions[i][k, :]
    end
    return off, rows
end

"""
    download_rows!(eng, floes, rows)

The resident state of the parents `rows` (1-based, any order, none twice) into those rows of the host list (`sz_download_rows`): columns,
geometry, sub-floe points, status and interactions, each value as `pull_state!` would give it -- the other floes are not touched and nothing
else crosses.  `pack` passes pointers to where the columns lie, so the named rows are packed from a contiguous copy (`floes[rows]`) and
written back row by row.  The fuse lists (`status.fuse_idx`) live on the host and are not part of this call.

Written, not run: there is no Julia on the machines this engine is built and tested on.  The C call underneath is held to the bits of a full
download by `tests/test_splice_gpu.py`.
"""
function download_rows!(eng::HIPEngine, floes, rows::AbstractVector{<:Integer})
    n = length(rows)
    n == 0 && return
    r0 = Int32.(rows .- 1)
    sizes = Vector{Int64}(undef, 3)
    check(eng, @ccall lib.sz_download_rows(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, r0::Ptr{Int32}, C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Int32},
                                           C_NULL::Ptr{Float64}, sizes::Ptr{Int64})::Cint)
    sub = floes[rows]
    P = pack(sub, n)
    resize!(P.vx, sizes[1]); resize!(P.vy, sizes[1]); resize!(P.sx, sizes[2]); resize!(P.sy, sizes[2])
    P.cols.vx = pointer(P.vx); P.cols.vy = pointer(P.vy); P.cols.sx = pointer(P.sx); P.cols.sy = pointer(P.sy)
    off = Vector{Int32}(undef, n + 1); irows = Matrix{Float64}(undef, 7, max(Int(sizes[3]), 1))
    GC.@preserve P sub begin
        check(eng, @ccall lib.sz_download_rows(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, r0::Ptr{Int32}, P.cols::Ref{SzFloeColumns}, off::Ptr{Int32},
                                               irows::Ptr{Float64}, C_NULL::Ptr{Int64})::Cint)
    end
    unpack_geometry!(sub, P); unpack_status!(sub, P)
    for k in 1:n
        s = P.sub_off[k]+1:P.sub_off[k+1]
        sub.x_subfloe_points[k] = P.sx[s]; sub.y_subfloe_points[k] = P.sy[s]
        r = off[k]+1:off[k+1]
        sub.interactions[k] = permutedims(irows[:, r]); sub.num_inters[k] = length(r)
        sub.collision_force[k][1, 1] = P.coll_fx[k]; sub.collision_force[k][1, 2] = P.coll_fy[k]
        floes[rows[k]] = sub[k]
    end
    return
end

"""
    splice!(eng, floes, del, rep, app_range)

The host's edit of a few floes into the resident list (`sz_splice_floes`), the other floes staying on the device.  `floes` is the host list with
the edit applied EXCEPT the deletion: the rows `rep` changed in place (`replace_floe!`, a fuse, a smoothed ring), the new floes appended at
`app_range` (pieces of a fracture or a ridge), the rows `del` still there -- so `del` and `rep` number host and device rows alike (1-based,
ascending, none in both).  Only the rows `rep` and `app_range` are packed (the existing `pack` on a contiguous copy of them) and uploaded with
their interactions; the rows `del` are then deleted from the host list as `deleteat!` does, and `eng.host_rows` is the identity again, as
after `upload!`.  Refused (the library's message is thrown, nothing has changed): ghosts in the list, a pending ridge / raft step, a tiled
context, rows that are unsorted, repeated or out of range.

`run_resident!` does not call this yet: it still makes the full round trip at a stop (`pull_state!`, `upload!`).

Written, not run: there is no Julia on the machines this engine is built and tested on.  The C call underneath is held, bit for bit, to an
upload of the edited list by `tests/test_splice_gpu.py`.
"""
function splice!(eng::HIPEngine, floes, del::AbstractVector{<:Integer}, rep::AbstractVector{<:Integer}, app_range::AbstractUnitRange{<:Integer})
    staged = vcat(collect(Int, rep), collect(Int, app_range))
    d0 = Int32.(del .- 1); r0 = Int32.(rep .- 1)
    if isempty(staged)
        check(eng, @ccall lib.sz_splice_floes(eng.ctx::Ptr{Cvoid}, Int32(length(d0))::Int32, d0::Ptr{Int32}, Int32(0)::Int32, C_NULL::Ptr{Int32},
                                              Int32(0)::Int32, C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Int32}, C_NULL::Ptr{Float64})::Cint)
    else
        sub = floes[staged]
        P = pack(sub, length(sub))
        off, irows = interactions_csr(sub)
        GC.@preserve P sub begin
            check(eng, @ccall lib.sz_splice_floes(eng.ctx::Ptr{Cvoid}, Int32(length(d0))::Int32, d0::Ptr{Int32}, Int32(length(r0))::Int32, r0::Ptr{Int32},
                                                  Int32(length(app_range))::Int32, P.cols::Ref{SzFloeColumns}, off::Ptr{Int32},
                                                  irows::Ptr{Float64})::Cint)
        end
    end
    for i in reverse(sort(collect(Int, del)))
        StructArrays.foreachfield(f -> deleteat!(f, i), floes)
    end
    eng.host_rows = collect(1:length(floes))
    return
end

# ------------------------------------------------------------------------------------------------ ridging and rafting
"""
    set_ridgeraft!(eng, sim)

The simulation's `RidgeRaftSettings` on the device (`sz_set_ridgeraft`): `Δt` and the five heights the gates of `timestep_ridging_rafting!`
(ridge_raft.jl:676-837) read.  A batch of `sz_step` then stops in the middle of a ridge / raft step (`mod(tstep, Δt) == 0`) whose candidate
table is not empty -- ghosts in the list, between `timestep_collisions!` and `timestep_ridging_rafting!` -- and runs through the others.
"""
function set_ridgeraft!(eng::HIPEngine, sim)
    rs = sim.ridgeraft_settings
    check(eng, @ccall lib.sz_set_ridgeraft(eng.ctx::Ptr{Cvoid}, Int32(rs.ridge_raft_on)::Int32, Int32(rs.Δt)::Int32,
                                           Float64(rs.min_ridge_height)::Float64, Float64(rs.max_floe_ridge_height)::Float64,
                                           Float64(rs.max_domain_ridge_height)::Float64, Float64(rs.max_floe_raft_height)::Float64,
                                           Float64(rs.max_domain_raft_height)::Float64)::Cint)
    return
end

# the timestep whose ridge / raft step is pending (sz_step stopped in its middle), or -1
function ridgeraft_pending(eng::HIPEngine)
    t = Ref{Int32}(-1)
    check(eng, @ccall lib.sz_ridgeraft_pending(eng.ctx::Ptr{Cvoid}, t::Ptr{Int32})::Cint)
    return Int(t[])
end

# per-floe draws of the ridge / raft steps the last sz_step ran through with an empty table
function ridgeraft_draws(eng::HIPEngine)
    n = Ref{Int64}(0)
    check(eng, @ccall lib.sz_ridgeraft_draws(eng.ctx::Ptr{Cvoid}, n::Ptr{Int64})::Cint)
    return Int(n[])
end

"""
    ridgeraft_candidates(eng) -> (i, j, kind, frac, n_draws)

The candidate table of the list as the device holds it (`sz_ridgeraft_candidates`; at a pending stop, or after `sz_add_ghosts` +
`sz_timestep_collisions`): `i` 1-based list rows, `j` the partner as `floe.interactions` names it, `kind` bit 1 ridge / bit 2 raft,
`frac = overlap / min_area`.
"""
function ridgeraft_candidates(eng::HIPEngine)
    n, nd = Ref{Int32}(0), Ref{Int64}(0)
    check(eng, @ccall lib.sz_ridgeraft_candidates(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, Int32(0)::Int32, C_NULL::Ptr{Int32}, C_NULL::Ptr{Int32},
                                                  C_NULL::Ptr{Int32}, C_NULL::Ptr{Float64}, nd::Ptr{Int64})::Cint)
    cap = max(Int(n[]), 1)
    i = Vector{Int32}(undef, cap); j = Vector{Int32}(undef, cap); k = Vector{Int32}(undef, cap); f = Vector{Float64}(undef, cap)
    check(eng, @ccall lib.sz_ridgeraft_candidates(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, Int32(cap)::Int32, i::Ptr{Int32}, j::Ptr{Int32},
                                                  k::Ptr{Int32}, f::Ptr{Float64}, nd::Ptr{Int64})::Cint)
    m = Int(n[])
    return (i = Int.(i[1:m]) .+ 1, j = Int.(j[1:m]), kind = Int.(k[1:m]), frac = f[1:m], n_draws = Int(nd[]))
end

"""
    ridgeraft_rows(eng) -> Vector{Int}

The list rows `timestep_ridging_rafting!` can touch (`sz_ridgeraft_rows`; where `ridgeraft_candidates` is valid): for every table entry row `i`
and, for a floe partner, row `j`, each with its root parent and every ghost on that parent's `ghosts` list -- ascending 1-based list rows, each
once; empty for an empty table.

Written, not run, as `download_rows!` and `splice!` are; the C call is held to the numpy statement of the rule by
`tests/test_pending_splice_gpu.py`.
"""
function ridgeraft_rows(eng::HIPEngine)
    n = Ref{Int32}(0)
    check(eng, @ccall lib.sz_ridgeraft_rows(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, Int32(0)::Int32, C_NULL::Ptr{Int32})::Cint)
    cap = max(Int(n[]), 1)
    rows = Vector{Int32}(undef, cap)
    check(eng, @ccall lib.sz_ridgeraft_rows(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, Int32(cap)::Int32, rows::Ptr{Int32})::Cint)
    return Int.(rows[1:Int(n[])]) .+ 1
end

"""
    download_list_rows!(eng, floes, rows)

`download_rows!` over the whole list (`sz_download_list_rows`): `floes` is the host list WITH its ghost rows (as `pull_state_with_ghosts!`
leaves it, one host row per list row) and `rows` may name any of them, 1-based, in any order, none twice.  A parent's `ghosts` come with it in
list numbers; a ghost row gets an empty list and no sub-floe points, as the reference's ghosts have them (`deepcopy_floe` copies the parent's
points, which nothing reads -- they are left as they are on the host).  The fuse lists are not part of this call.

Written, not run: there is no Julia on the machines this engine is built and tested on.  The C call underneath is held to the bits of a full
download by `tests/test_pending_splice_gpu.py`.
"""
function download_list_rows!(eng::HIPEngine, floes, rows::AbstractVector{<:Integer})
    n = length(rows)
    n == 0 && return
    r0 = Int32.(rows .- 1)
    sizes = Vector{Int64}(undef, 3)
    check(eng, @ccall lib.sz_download_list_rows(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, r0::Ptr{Int32}, C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Int32},
                                                C_NULL::Ptr{Float64}, sizes::Ptr{Int64})::Cint)
    sub = floes[rows]
    P = pack(sub, n)
    resize!(P.vx, sizes[1]); resize!(P.vy, sizes[1]); resize!(P.sx, sizes[2]); resize!(P.sy, sizes[2]); resize!(P.ghost_idx, 3n)
    P.cols.vx = pointer(P.vx); P.cols.vy = pointer(P.vy); P.cols.sx = pointer(P.sx); P.cols.sy = pointer(P.sy)
    P.cols.ghost_off = pointer(P.ghost_off); P.cols.ghost_idx = pointer(P.ghost_idx)
    off = Vector{Int32}(undef, n + 1); irows = Matrix{Float64}(undef, 7, max(Int(sizes[3]), 1))
    GC.@preserve P sub begin
        check(eng, @ccall lib.sz_download_list_rows(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, r0::Ptr{Int32}, P.cols::Ref{SzFloeColumns}, off::Ptr{Int32},
                                                    irows::Ptr{Float64}, C_NULL::Ptr{Int64})::Cint)
    end
    unpack_geometry!(sub, P); unpack_status!(sub, P)
    sub.id .= P.id; sub.ghost_id .= P.ghost_id
    for k in 1:n
        if sub.ghost_id[k] == 0          # (a parent: its points and its ghost list are the device's)
            s = P.sub_off[k]+1:P.sub_off[k+1]
            sub.x_subfloe_points[k] = P.sx[s]; sub.y_subfloe_points[k] = P.sy[s]
        end
        sub.ghosts[k] = Int.(P.ghost_idx[P.ghost_off[k]+1:P.ghost_off[k+1]]) .+ 1
        r = off[k]+1:off[k+1]
        sub.interactions[k] = permutedims(irows[:, r]); sub.num_inters[k] = length(r)
        sub.collision_force[k][1, 1] = P.coll_fx[k]; sub.collision_force[k][1, 2] = P.coll_fy[k]
        floes[rows[k]] = sub[k]
    end
    return
end

"""
    splice_parents!(eng, floes, n_parents, del, rep, app_range)

`splice!` at a stop that still has its ghosts in the list (`sz_splice_parents`): a pending ridge / raft step.  `floes` is the host list as
`timestep_ridging_rafting!` left it -- `n_parents` parents, then the ghosts, then the pieces it collected at `app_range` -- with the rows `rep`
of the parents changed in place and the rows `del` still there.  The device drops its ghosts as `sz_remove_ghosts` does and applies the edit to
the parents; the pending step stays pending (`sz_step_finish` runs its second half).  The host list follows `timestep_sim!`
(simulation.jl:137-147): the ghost rows go, the pieces stay behind the parents, the rows `del` are deleted.

Written, not run.  The C call underneath is held, bit for bit, to `sz_remove_ghosts` + an upload of the edited parents by
`tests/test_pending_splice_gpu.py`.
"""
function splice_parents!(eng::HIPEngine, floes, n_parents::Integer, del::AbstractVector{<:Integer}, rep::AbstractVector{<:Integer},
                         app_range::AbstractUnitRange{<:Integer})
    staged = vcat(collect(Int, rep), collect(Int, app_range))
    d0 = Int32.(del .- 1); r0 = Int32.(rep .- 1)
    if isempty(staged)
        check(eng, @ccall lib.sz_splice_parents(eng.ctx::Ptr{Cvoid}, Int32(length(d0))::Int32, d0::Ptr{Int32}, Int32(0)::Int32, C_NULL::Ptr{Int32},
                                                Int32(0)::Int32, C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Int32}, C_NULL::Ptr{Float64})::Cint)
    else
        sub = floes[staged]
        P = pack(sub, length(sub))
        off, irows = interactions_csr(sub)
        GC.@preserve P sub begin
            check(eng, @ccall lib.sz_splice_parents(eng.ctx::Ptr{Cvoid}, Int32(length(d0))::Int32, d0::Ptr{Int32}, Int32(length(r0))::Int32,
                                                    r0::Ptr{Int32}, Int32(length(app_range))::Int32, P.cols::Ref{SzFloeColumns}, off::Ptr{Int32},
                                                    irows::Ptr{Float64})::Cint)
        end
    end
    isempty(d0) && isempty(staged) && return          # (the library changed nothing and dropped no ghost)
    gone = sort(unique(vcat(collect(Int, del), [i for i in n_parents+1:length(floes) if !(i in app_range)])))
    for i in reverse(gone)
        StructArrays.foreachfield(f -> deleteat!(f, i), floes)
    end
    for i in eachindex(floes.ghosts)
        empty!(floes.ghosts[i])
    end
    eng.host_rows = collect(1:length(floes))
    return
end

# ... for a Floe{Float32} host (see "Float32 hosts" below): the same calls through the _f32 twins on the columns of pack32.  ridgeraft_rows32
# names the call a Float32 host finds under the suffix; no floating-point value crosses it.
function ridgeraft_rows32(eng::HIPEngine)
    n = Ref{Int32}(0)
    check(eng, @ccall lib.sz_ridgeraft_rows_f32(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, Int32(0)::Int32, C_NULL::Ptr{Int32})::Cint)
    cap = max(Int(n[]), 1)
    rows = Vector{Int32}(undef, cap)
    check(eng, @ccall lib.sz_ridgeraft_rows_f32(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, Int32(cap)::Int32, rows::Ptr{Int32})::Cint)
    return Int.(rows[1:Int(n[])]) .+ 1
end

# the list rows `rows` into a contiguous copy of them: (copy, its Packed32 -- the flattened columns hold the device's values, as after
# download32! --, ghost_off, ghost_idx, inter_off, inter_rows 7 x k)
function download_list_rows32(eng::HIPEngine, floes::StructArray{<:Floe{Float32}}, rows::AbstractVector{<:Integer})
    n = length(rows)
    r0 = Int32.(rows .- 1)
    sizes = Vector{Int64}(undef, 3)
    check(eng, @ccall lib.sz_download_list_rows_f32(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, r0::Ptr{Int32}, C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Int32},
                                                    C_NULL::Ptr{Float32}, sizes::Ptr{Int64})::Cint)
    sub = floes[rows]
    P = pack32(sub, n)
    vx = Vector{Float32}(undef, sizes[1]); vy = similar(vx); sx = Vector{Float32}(undef, sizes[2]); sy = similar(sx)
    goff = Vector{Int32}(undef, n + 1); gidx = Vector{Int32}(undef, max(3n, 1))
    P.cols.vx = pointer(vx); P.cols.vy = pointer(vy); P.cols.sx = pointer(sx); P.cols.sy = pointer(sy)
    P.cols.ghost_off = pointer(goff); P.cols.ghost_idx = pointer(gidx)
    append!(P.keep, Any[vx, vy, sx, sy, goff, gidx])
    off = Vector{Int32}(undef, n + 1); irows = Matrix{Float32}(undef, 7, max(Int(sizes[3]), 1))
    GC.@preserve P sub begin
        check(eng, @ccall lib.sz_download_list_rows_f32(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, r0::Ptr{Int32}, P.cols::Ref{SzFloeColumnsF32},
                                                        off::Ptr{Int32}, irows::Ptr{Float32}, C_NULL::Ptr{Int64})::Cint)
    end
    return sub, P, goff, gidx[1:goff[end]], off, irows
end

# sz_splice_parents_f32 with the rows `rep` and `app_range` of the host list packed by pack32; the host list is the caller's to follow
function splice_parents32!(eng::HIPEngine, floes::StructArray{<:Floe{Float32}}, del::AbstractVector{<:Integer}, rep::AbstractVector{<:Integer},
                           app_range::AbstractUnitRange{<:Integer})
    staged = vcat(collect(Int, rep), collect(Int, app_range))
    isempty(staged) && error("splice_parents32!: nothing replaced or appended (a deletion alone needs no columns: splice_parents!)")
    d0 = Int32.(del .- 1); r0 = Int32.(rep .- 1)
    sub = floes[staged]
    P = pack32(sub, length(sub))
    off = Vector{Int32}(undef, length(sub) + 1); off[1] = 0
    for i in 1:length(sub)
        off[i+1] = off[i] + sub.num_inters[i]
    end
    irows = Matrix{Float32}(undef, 7, max(Int(off[end]), 1))
    for i in 1:length(sub), k in 1:sub.num_inters[i]
        irows[:, off[i]+k] .= @view sub.interactions[i][k, :]
    end
    GC.@preserve P sub begin
        check(eng, @ccall lib.sz_splice_parents_f32(eng.ctx::Ptr{Cvoid}, Int32(length(d0))::Int32, d0::Ptr{Int32}, Int32(length(r0))::Int32,
                                                    r0::Ptr{Int32}, Int32(length(app_range))::Int32, P.cols::Ref{SzFloeColumnsF32},
                                                    off::Ptr{Int32}, irows::Ptr{Float32})::Cint)
    end
    return
end

# At a pending stop the device list holds the ghosts: the host rows follow the parents (pull_state!'s removal bookkeeping), then one row per
# device ghost is appended -- a copy of its parent, overwritten by the download -- with the ghost lists, ids and ghost ids of the device.
function pull_state_with_ghosts!(eng::HIPEngine, floes, P::Packed, ocean = nothing)
    st = stats(eng)
    M, N = Int(st.M), Int(st.N)
    o = origin(eng)
    if length(o) != length(floes) && length(eng.host_rows) == length(floes)
        named = Set(o)
        for i in reverse(eachindex(eng.host_rows))
            eng.host_rows[i] in named && continue
            StructArrays.foreachfield(f -> deleteat!(f, i), floes)
            deleteat!(eng.host_rows, i)
        end
    end
    length(floes) == N || error("pull_state_with_ghosts!: the host holds $(length(floes)) parents, the device $N")
    goff = Vector{Int32}(undef, M + 1); gidx = Vector{Int32}(undef, max(3M, 1))
    only = SzFloeColumns()
    only.ghost_off = pointer(goff); only.ghost_idx = pointer(gidx)
    GC.@preserve goff gidx begin
        check(eng, @ccall lib.sz_download_floes(eng.ctx::Ptr{Cvoid}, only::Ref{SzFloeColumns})::Cint)
    end
    parent_of = zeros(Int, M)
    for i in 1:N, g in gidx[goff[i]+1:goff[i+1]]
        parent_of[g+1] = i
    end
    for g in N+1:M
        parent_of[g] > 0 || error("pull_state_with_ghosts!: ghost row $g has no parent")
        push!(floes, Subzero.deepcopy_floe(LazyRow(floes, parent_of[g])))
    end
    for i in 1:M
        floes.ghosts[i] = i <= N ? Int.(gidx[goff[i]+1:goff[i+1]]) .+ 1 : Int[]
    end
    isnothing(ocean) || pull_dissolved!(eng, ocean)
    P = pack(floes, N)
    download!(eng, floes, P)
    unpack_geometry!(floes, P); unpack_status!(floes, P)
    floes.id .= P.id; floes.ghost_id .= P.ghost_id
    off = Vector{Int32}(undef, M + 1); rows = Matrix{Float64}(undef, 7, max(Int(st.n_inter_rows), 1))
    check(eng, @ccall lib.sz_download_interactions(eng.ctx::Ptr{Cvoid}, off::Ptr{Int32}, rows::Ptr{Float64})::Cint)
    foff = Vector{Int32}(undef, M + 1)
    check(eng, @ccall lib.sz_download_fuse(eng.ctx::Ptr{Cvoid}, foff::Ptr{Int32}, C_NULL::Ptr{Int32})::Cint)
    fidx = Vector{Int32}(undef, max(Int(foff[end]), 1))
    check(eng, @ccall lib.sz_download_fuse(eng.ctx::Ptr{Cvoid}, foff::Ptr{Int32}, fidx::Ptr{Int32})::Cint)
    for i in 1:M
        r = off[i]+1:off[i+1]
        floes.interactions[i] = permutedims(rows[:, r]); floes.num_inters[i] = length(r)
        floes.collision_force[i][1, 1] = P.coll_fx[i]; floes.collision_force[i][1, 2] = P.coll_fy[i]
        empty!(floes.status[i].fuse_idx); append!(floes.status[i].fuse_idx, Int.(fidx[foff[i]+1:foff[i+1]]) .+ 1)
    end
    return N
end

# ------------------------------------------------------------------------------------------------ resident mode
"""
    run_resident!(sim, eng; start_tstep = 0, batch = 500)

`run!(sim)` for simulations in which only the hot path, ridging / rafting, fracture and welding touch the floes between output steps.
Whole batches of `timestep_sim!` run on the device with the state resident in
HBM (`sz_step`); a batch never crosses an output step of a writer, and it ends after the first step that leaves a floe
tagged `remove` / `fuse`, so `simplify_floes!` (simulation.jl:205-214) runs exactly where the reference runs it.
`sz_simplify_check` covers its other two triggers (rings over `max_vertices`, floes under the minimum area / height).

Fractures (`FractureSettings.fractures_on` with a `HiblerYieldCurve` or `MohrsCone` criterion and a `DecayAreaScaledCalculator`):
the device evaluates `determine_fractures` after every fracture step (`mod(tstep, Δt) == 0`) and a batch also ends after the
first fracture step on which a floe would fracture.  The state is then pulled, `fracture_floes!` runs on the host exactly as
`timestep_sim!` calls it (simulation.jl:172-183), then `simplify_floes!`, and the batch resumes from the uploaded state.  On
fracture steps without a candidate `fracture_floes!` would change nothing and is skipped: `determine_fractures` draws no random
numbers, so `sim.rng` stays exactly where the reference leaves it.

Welding (`WeldSettings.weld_on`): on a welding step (`findfirst(x -> mod(tstep, x) == 0, Δts)`, simulation.jl:184-202) the device computes the
overlap table of the pairs `timestep_welding!` would clip, and a batch also ends after the first welding step whose table is not empty.  The
state is then pulled and `timestep_welding!(floes, max_floe_id, table, ...)` of this module welds from the table, then `simplify_floes!` as in
the reference.  With an empty table the reference's call changes nothing and draws no random number; it is skipped.  The reference hands
`timestep_welding!` no `rng` (a fresh `Xoshiro()` per call), and so does this loop.

Ridging and rafting (`RidgeRaftSettings.ridge_raft_on`): on a ridge / raft step (`mod(tstep, Δt) == 0`, simulation.jl:121-136) the device runs
the step's first half (`add_ghosts!`, `timestep_collisions!`) and evaluates the candidate table: the gates of `timestep_ridging_rafting!` with
every random draw assumed to pass.  With an empty table the reference's call changes no floe and draws exactly the per-floe numbers
(ridge_raft.jl:694-697); the batch runs on and, after every `sz_step`, `sim.rng` is advanced by `sz_ridgeraft_draws` calls of `rand(sim.rng,
FT)` before any host process of that batch end uses it.  With candidates the batch stops in the middle of the step: the state is pulled
WITH its ghosts, `Subzero.timestep_ridging_rafting!` runs unchanged with `sim.rng` and a fresh pieces buffer, the ghosts are removed and the
pieces appended as simulation.jl:137-147 does, the floes and their interactions are uploaded, `sz_step_finish` runs the rest of the step,
and the step ends like any other (fracture, weld, simplify).

Removal (`set_removal!`): where `simplify_floes!` reduces to `remove_floes!` -- nothing to fuse, no ring to smooth -- the device deletes the
rows and adds the dissolved mass to its copy of `ocean.dissolved`, inside a batch (which then runs on) or, behind a batch's last step, through
`remove_floes!(eng)`.  The host's rows follow at the next `pull_state!`, which deletes the rows `origin(eng)` no longer names.

Output (`device_output = true`; off by default, this file has not been run): every GridOutputWriter and every FloeOutputWriter whose outputs a
frame serves (`frame_covers`: every field of `Floe`, so the default `FloeOutputWriter(Δtout)` too) is registered with the recorder
(`set_floe_output!`, `set_grid_output!`; four of each at most).  Batches then run past those writers' output steps -- `sz_step` cuts before
the step, records the frames on the device and goes on -- and `drain_frames!` writes them through the writers' own files after each batch.
Every other writer (checkpoint, initial state, a fifth writer) keeps the cut on the host, where only those writers write.
"""
function run_resident!(sim, eng::HIPEngine; start_tstep::Integer = 0, batch::Integer = 500, device_output::Bool = false)
    # (the candidates are read from the step's own interaction rows: sz_step refuses ridge / raft without SZ_COLLISIONS_ON)
    sim.ridgeraft_settings.ridge_raft_on && !sim.collision_settings.collisions_on &&
        error("run_resident!: ridging / rafting with collisions off works on rows no step refreshes: use run!(sim)")
    set_ridgeraft!(eng, sim)
    set_fracture!(eng, sim)
    set_welding!(eng, sim)
    set_removal!(eng, sim)
    if device_output
        for i in eachindex(sim.writers.floewriters)
            set_floe_output!(eng, sim, i)
        end
        for i in eachindex(sim.writers.gridwriters)
            set_grid_output!(eng, sim, i)
        end
    end
    rec = device_output ? eng : nothing
    fractures = sim.fracture_settings.fractures_on
    ws = sim.weld_settings
    Subzero.startup_sim(sim, nothing, 1)
    floes = sim.model.floes
    flags = (sim.collision_settings.collisions_on ? SZ_COLLISIONS_ON : Int32(0)) |
            (sim.coupling_settings.coupling_on ? SZ_COUPLING_ON : Int32(0))
    max_floe_id = isempty(floes) ? 0 : maximum(floes.id)
    P = upload!(eng, floes, length(floes))
    upload_interactions!(eng, floes)
    push_dissolved!(eng, sim.model.ocean)
    ocean = sim.model.ocean
    tstep, last = start_tstep, start_tstep + sim.nΔt
    dirty = false                                    # the device state is ahead of the host's
    while tstep <= last
        if output_due(sim.writers, tstep, start_tstep, rec)
            dirty && (P = pull_state!(eng, floes, P, ocean); dirty = false)
            Subzero.add_ghosts!(floes, sim.model.domain)           # write_data! sees the ghosts (simulation.jl:102-105)
            device_output ? write_host_data!(sim, eng, tstep, start_tstep) : Subzero.write_data!(sim, tstep, start_tstep)
            remove_ghosts!(floes)
        end
        n = min(batch, last - tstep + 1, steps_to_next_output(sim.writers, tstep, start_tstep, rec))
        done = Ref{Int32}(0)
        check(eng, @ccall lib.sz_step(eng.ctx::Ptr{Cvoid}, n::Int32, tstep::Int32, sim.Δt::Int32,
                                      sim.coupling_settings.Δt::Int32, flags::Int32, done::Ptr{Int32})::Cint)
        tstep += done[]; dirty = true
        # the frames of the output steps the batch began: through the writers' files.  A batch that ended on a frame without room goes on
        # from that step with the frames cleared
        device_output && drain_frames!(eng, sim)
        # ridge / raft steps the batch ran through with an empty table: their per-floe draws, before anything below uses sim.rng
        if sim.ridgeraft_settings.ridge_raft_on
            for _ in 1:ridgeraft_draws(eng)
                rand(sim.rng, Float64)
            end
        end
        # the batch stopped in the middle of a ridge / raft step with candidates: the reference's own function on the pulled list, then the
        # rest of the step on the device
        stepped = done[] > 0
        if sim.ridgeraft_settings.ridge_raft_on && ridgeraft_pending(eng) >= 0
            pend = ridgeraft_pending(eng)
            pull_state_with_ghosts!(eng, floes, P, ocean)
            pieces = StructArray{Floe{Float64}}(undef, 0)
            max_floe_id = Subzero.timestep_ridging_rafting!(floes, pieces, sim.model.domain, max_floe_id, sim.ridgeraft_settings,
                                                            sim.floe_settings, sim.simp_settings, sim.Δt, sim.rng)
            remove_ghosts!(floes)
            append!(floes, pieces)
            P = upload!(eng, floes, length(floes)); upload_interactions!(eng, floes)
            check(eng, @ccall lib.sz_step_finish(eng.ctx::Ptr{Cvoid}, Int32(pend)::Int32, sim.Δt::Int32, sim.coupling_settings.Δt::Int32,
                                                 flags::Int32)::Cint)
            tstep = pend + 1; stepped = true
        end
        # the batch's last step was a fracture step on which a floe fractures: fracture_floes! on the host, before simplify_floes!
        fracture_now = fractures && stepped && mod(tstep - 1, sim.fracture_settings.Δt) == 0 && fracture_candidates(eng) > 0
        if fracture_now
            P = pull_state!(eng, floes, P, ocean)
            max_floe_id = Subzero.fracture_floes!(floes, max_floe_id, sim.rng, sim.fracture_settings, sim.floe_settings, sim.Δt)
        end
        # ... and a welding step: the table of the floes as they are now (behind fracture_floes!, as in timestep_sim!), welded on the host
        weld_idx = sim.weld_settings.weld_on && stepped ? findfirst(x -> mod(tstep - 1, x) == 0, ws.Δts) : nothing
        weld_now = false
        if !isnothing(weld_idx)
            if fracture_now          # the device still holds the floes from before fracture_floes!
                P = upload!(eng, floes, length(floes)); upload_interactions!(eng, floes)
            end
            table = weld_overlaps(eng, ws.Nxs[weld_idx], ws.Nys[weld_idx], ws.max_weld_area)
            if !isempty(table.i)
                fracture_now || (P = pull_state!(eng, floes, P, ocean))
                max_floe_id = timestep_welding!(floes, max_floe_id, table, ws, sim.floe_settings, weld_idx, sim.Δt)
                weld_now = true
            end
        end
        host_ahead = fracture_now || weld_now
        todo = Vector{Int64}(undef, 4)
        host_ahead || check(eng, @ccall lib.sz_simplify_check(eng.ctx::Ptr{Cvoid}, eng.max_vertices::Int32, eng.min_floe_area::Float64,
                                                              eng.min_floe_height::Float64, todo::Ptr{Int64})::Cint)
        # only removals and dissolutions (nothing to fuse, no ring to smooth): the device's pass instead of pull, simplify_floes!, upload
        if !host_ahead && any(!iszero, todo) && todo[2] == 0 && todo[3] == 0 && remove_floes!(eng).done
            todo .= 0
        end
        if host_ahead || any(!iszero, todo)        # simplify_floes! has work: it runs on the host, on the full state
            host_ahead || (P = pull_state!(eng, floes, P, ocean))
            max_floe_id = Subzero.simplify_floes!(sim.model, max_floe_id, sim.simp_settings, sim.collision_settings,
                                                  sim.floe_settings, sim.Δt, sim.rng)
            P = upload!(eng, floes, length(floes)); upload_interactions!(eng, floes)
            push_dissolved!(eng, ocean)
            dirty = false
        end
    end
    dirty && (P = pull_state!(eng, floes, P, ocean))
    sim.coupling_settings.two_way_coupling_on && pull_ocean_stress!(eng, sim.model.ocean)
    pull_moving_boundaries!(eng, sim.model.domain)
    Subzero.teardown_sim(sim)
    return
end

# the whole floe state back into the StructArray (columns, geometry, interactions, status + fuse lists).  The device may have removed floes
# since the upload (set_removal!): the host rows `origin` no longer names go first, `P` is made again for the rows that stay (the returned one
# replaces the caller's), and the running ocean.dissolved lattice comes back with the floes.
function pull_state!(eng::HIPEngine, floes, P::Packed, ocean = nothing)
    o = origin(eng)
    if length(o) != length(floes) && length(eng.host_rows) == length(floes)
        named = Set(o)
        for i in reverse(eachindex(eng.host_rows))
            eng.host_rows[i] in named && continue
            StructArrays.foreachfield(f -> deleteat!(f, i), floes)
            deleteat!(eng.host_rows, i)
        end
        P = pack(floes, length(floes))
    end
    isnothing(ocean) || pull_dissolved!(eng, ocean)
    M = length(floes)
    download!(eng, floes, P)
    unpack_geometry!(floes, P); unpack_status!(floes, P)
    st = stats(eng)
    off = Vector{Int32}(undef, M + 1); rows = Matrix{Float64}(undef, 7, max(Int(st.n_inter_rows), 1))
    check(eng, @ccall lib.sz_download_interactions(eng.ctx::Ptr{Cvoid}, off::Ptr{Int32}, rows::Ptr{Float64})::Cint)
    foff = Vector{Int32}(undef, M + 1)
    check(eng, @ccall lib.sz_download_fuse(eng.ctx::Ptr{Cvoid}, foff::Ptr{Int32}, C_NULL::Ptr{Int32})::Cint)
    fidx = Vector{Int32}(undef, max(Int(foff[end]), 1))
    check(eng, @ccall lib.sz_download_fuse(eng.ctx::Ptr{Cvoid}, foff::Ptr{Int32}, fidx::Ptr{Int32})::Cint)
    for i in 1:M
        r = off[i]+1:off[i+1]
        floes.interactions[i] = permutedims(rows[:, r]); floes.num_inters[i] = length(r)
        floes.collision_force[i][1, 1] = P.coll_fx[i]; floes.collision_force[i][1, 2] = P.coll_fy[i]
        empty!(floes.status[i].fuse_idx); append!(floes.status[i].fuse_idx, Int.(fidx[foff[i]+1:foff[i+1]]) .+ 1)
    end
    return P
end

# ghost rows off again (simulation.jl:138-144)
function remove_ghosts!(floes)
    n = count(==(0), floes.ghost_id)
    for i in reverse(n+1:length(floes))
        StructArrays.foreachfield(f -> deleteat!(f, i), floes)
    end
    empty!.(floes.ghosts)
    return
end

# ------------------------------------------------------------------------------------------------ tiles: one process per GPU
# A tiled run (DESIGN.md §6): every rank owns the floes of one spatial tile and trades a one-deep halo of ghost-floe records
# with the neighbouring tiles each step, inside the library.  Between the ranks the library uses either RCCL (it opens the
# communicator itself from a 128-byte id the host hands round) or the host's OWN channel -- three blocking collectives on
# host memory, e.g. MPI.jl calls -- for hosts without a device-aware MPI or with several ranks on one GPU.

# include/subzero_hip.h: sz_host_transport
struct SzHostTransport
    user::Ptr{Cvoid}
    allgather::Ptr{Cvoid}
    sendrecv::Ptr{Cvoid}
    allreduce_sum_f64::Ptr{Cvoid}
end

# the host program's collectives: (allgather!(recv::Vector{UInt8}, send::Vector{UInt8}),
#                                  sendrecv!(peers::Vector{Int32}, send::Vector{Vector{UInt8}}, recv::Vector{Vector{UInt8}}),
#                                  allreduce_sum!(buf::Vector{Float64})), e.g. with MPI.jl:
#     allgather!(r, s)       = MPI.Allgather!(s, MPI.UBuffer(r, length(s)), comm)
#     sendrecv!(p, s, r)     = MPI.Waitall(vcat([MPI.Irecv!(r[k], comm; source = p[k], tag = 7) for k in eachindex(p) if !isempty(r[k])],
#                                                [MPI.Isend(s[k], comm; dest = p[k], tag = 7) for k in eachindex(p) if !isempty(s[k])]))
#     allreduce_sum!(b)      = MPI.Allreduce!(b, +, comm)
const TRANSPORT = Ref{Any}(nothing)
const TRANSPORT_NRANKS = Ref{Int}(1)

function _transport_allgather(user::Ptr{Cvoid}, send::Ptr{UInt8}, recv::Ptr{UInt8}, bytes::Int64)::Cint
    try
        TRANSPORT[][1](unsafe_wrap(Array, recv, bytes * TRANSPORT_NRANKS[]), unsafe_wrap(Array, send, bytes))
        return Cint(0)
    catch
        return Cint(1)                               # (an exception must not unwind through the C frames)
    end
end
function _transport_sendrecv(user::Ptr{Cvoid}, npeers::Int32, peer::Ptr{Int32}, send::Ptr{Ptr{UInt8}}, send_bytes::Ptr{Int64},
                             recv::Ptr{Ptr{UInt8}}, recv_bytes::Ptr{Int64})::Cint
    try
        n = Int(npeers)
        peers = unsafe_wrap(Array, peer, n); sb = unsafe_wrap(Array, send_bytes, n); rb = unsafe_wrap(Array, recv_bytes, n)
        sp = unsafe_wrap(Array, send, n); rp = unsafe_wrap(Array, recv, n)
        TRANSPORT[][2](copy(peers), [unsafe_wrap(Array, sp[k], sb[k]) for k in 1:n], [unsafe_wrap(Array, rp[k], rb[k]) for k in 1:n])
        return Cint(0)
    catch
        return Cint(1)
    end
end
function _transport_allreduce(user::Ptr{Cvoid}, buf::Ptr{Float64}, n::Int64)::Cint
    try
        TRANSPORT[][3](unsafe_wrap(Array, buf, n))
        return Cint(0)
    catch
        return Cint(1)
    end
end

"""
    tiles!(eng, nranks, rank, owned_global_index, max_ring, max_rmax, Lx, Ly; id = nothing, transport = nothing,
           periodic_x = true, periodic_y = true, drift_margin = max(2000.0, max_rmax / 2), rebox_every = 150)

Collective, after `upload!` of the floes this rank owns (those whose centroid lies in its tile; `owned_global_index[i]` =
the index floe `i` has in the whole field, `max_ring` / `max_rmax` over ALL floes: halo floes arrive unseen).  `id`: the 128
bytes of `comm_unique_id()` from rank 0, handed round by the host (RCCL between the ranks); `transport` = the three
collectives described above (the host's channel).  Then `tile_run!` replaces `sz_step`.
"""
function tiles!(eng::HIPEngine, nranks::Integer, rank::Integer, owned_global_index::Vector{Int64}, max_ring::Real, max_rmax::Real,
                Lx::Real, Ly::Real; id = nothing, transport = nothing, periodic_x::Bool = true, periodic_y::Bool = true,
                drift_margin::Real = max(2000.0, max_rmax / 2), rebox_every::Integer = 150, tile_center = nothing)
    if transport !== nothing
        TRANSPORT[] = transport; TRANSPORT_NRANKS[] = nranks
        t = Ref(SzHostTransport(C_NULL,
            @cfunction(_transport_allgather, Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{UInt8}, Int64)),
            @cfunction(_transport_sendrecv, Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Ptr{UInt8}}, Ptr{Int64}, Ptr{Ptr{UInt8}}, Ptr{Int64})),
            @cfunction(_transport_allreduce, Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64))))
        check(eng, @ccall lib.sz_comm_init_host(eng.ctx::Ptr{Cvoid}, nranks::Int32, rank::Int32, t::Ptr{SzHostTransport})::Cint)
    else
        idp = id === nothing ? C_NULL : pointer(id)
        GC.@preserve id check(eng, @ccall lib.sz_comm_init(eng.ctx::Ptr{Cvoid}, nranks::Int32, rank::Int32, idp::Ptr{Cvoid})::Cint)
    end
    check(eng, @ccall lib.sz_tile_enable(eng.ctx::Ptr{Cvoid}, owned_global_index::Ptr{Int64}, Float64(max_ring)::Float64,
                                         Float64(max_rmax)::Float64)::Cint)
    check(eng, @ccall lib.sz_tile_setup(eng.ctx::Ptr{Cvoid}, Float64(Lx)::Float64, Float64(Ly)::Float64, Int32(periodic_x)::Int32,
                                        Int32(periodic_y)::Int32, Float64(drift_margin)::Float64, Int32(rebox_every)::Int32)::Cint)
    if tile_center !== nothing           # (x, y) of this rank's tile centre: see sz_tile_set_center
        check(eng, @ccall lib.sz_tile_set_center(eng.ctx::Ptr{Cvoid}, Float64(tile_center[1])::Float64, Float64(tile_center[2])::Float64)::Cint)
    end
    return
end

function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    @ccall(lib.sz_comm_unique_id(id::Ptr{Cvoid})::Cint) == 0 || error("sz_comm_unique_id: RCCL could not be bound")
    return id
end

# nsteps x timestep_sim! of the tiled run, collectively (same arguments on every rank).  Returns the steps run: like sz_step the batch
# ends after the first step that leaves a floe tagged remove / fuse on ANY rank (the same number on every rank), so that the host's
# simplify_floes! runs at the step the reference runs it (simulation.jl:205-214).  With a criterion set (`set_fracture!`: fractures need
# not be turned off for a tiled run) it also ends after the first fracture step on which a floe of ANY rank would fracture; the batch's
# own last step is not looked at -- `tile_fracture_candidates` answers for it.  With welding set (`set_welding!`) it likewise ends after the
# first welding step whose overlap table of the global list is not empty (`tile_weld_overlaps`)
function tile_run!(eng::HIPEngine, nsteps::Integer, tstep::Integer, Δt::Integer, coupling_Δt::Integer, flags::Integer)
    done = Ref{Int32}(0)
    check(eng, @ccall lib.sz_tile_run(eng.ctx::Ptr{Cvoid}, nsteps::Int32, tstep::Int32, Δt::Int32, coupling_Δt::Int32, flags::Int32,
                                      done::Ptr{Int32})::Cint)
    return Int(done[])
end

# determine_fractures over the global floe list whose rows live on the ranks' tiles (sz_tile_fracture_candidates): collective, on the state
# as it is.  Returns (candidates on all ranks -- the same number on every rank, 1-based local rows of this rank's candidates ascending, their
# 0-based global indices).  Mean height, p and verdicts are the undivided list's, to the bit.
function tile_fracture_candidates(eng::HIPEngine, n_owned::Integer)
    ng = Ref{Int32}(0); no = Ref{Int32}(0)
    rows = Vector{Int32}(undef, max(n_owned, 1)); g = Vector{Int64}(undef, max(n_owned, 1))
    check(eng, @ccall lib.sz_tile_fracture_candidates(eng.ctx::Ptr{Cvoid}, ng::Ptr{Int32}, no::Ptr{Int32}, rows::Ptr{Int32}, g::Ptr{Int64})::Cint)
    return Int(ng[]), Int.(rows[1:no[]]) .+ 1, g[1:no[]]
end

# the welding overlap table of the global floe list whose rows live on the ranks' tiles (sz_tile_weld_overlaps): collective, on the state as it
# is.  Returns (i, j, inter_area) with 1-based GLOBAL numbers i < j, the whole table on every rank: the rows `weld_overlaps` gives for the
# undivided list, in its order, areas to the bit.  `tile_run!` with `set_welding!` ends after the first welding step whose table is not empty;
# its own last step is not looked at -- this answers for it
function tile_weld_overlaps(eng::HIPEngine, nx::Integer, ny::Integer, max_weld_area::Real)
    n = Ref{Int32}(0)
    check(eng, @ccall lib.sz_tile_weld_overlaps(eng.ctx::Ptr{Cvoid}, Int32(nx)::Int32, Int32(ny)::Int32, Float64(max_weld_area)::Float64, n::Ptr{Int32},
                                                Int32(0)::Int32, C_NULL::Ptr{Int64}, C_NULL::Ptr{Int64}, C_NULL::Ptr{Float64})::Cint)
    cap = max(Int(n[]), 1)
    i = Vector{Int64}(undef, cap); j = Vector{Int64}(undef, cap); a = Vector{Float64}(undef, cap)
    check(eng, @ccall lib.sz_tile_weld_overlaps(eng.ctx::Ptr{Cvoid}, Int32(nx)::Int32, Int32(ny)::Int32, Float64(max_weld_area)::Float64, n::Ptr{Int32},
                                                Int32(cap)::Int32, i::Ptr{Int64}, j::Ptr{Int64}, a::Ptr{Float64})::Cint)
    return i[1:n[]] .+ 1, j[1:n[]] .+ 1, a[1:n[]]
end

# Ridging and rafting in a tiled run (written against the C-ABI and not run: no Julia was available).  `tile_set_ridgeraft!` puts the simulation's
# RidgeRaftSettings on this rank's context (the same on every rank); `tile_run!` then stops on every rank in the middle of the first ridge / raft
# step whose candidate table of the global list is not empty: the step is not counted, `ridgeraft_pending(eng)` names it, the lists keep their
# halo rows and ghosts, and `tile_run!` / `tile_migrate!` refuse until `tile_step_finish!` has run.  Steps with an empty table are run through;
# `ridgeraft_draws(eng)` is the sum over the ranks, by which EVERY rank advances its copy of sim.rng.  The host's side of a non-empty table on tiles
# -- gathering the list, timestep_ridging_rafting!, handing the floes back to their tiles -- is not written yet (DESIGN.md §10): these calls give
# that host the table, the list numbers and the finish.
function tile_set_ridgeraft!(eng::HIPEngine, sim)
    set_ridgeraft!(eng, sim)
    return
end

# at a pending stop (collective): (i, j, kind, frac, n_draws) of the global list, the whole table on every rank, as `ridgeraft_candidates` gives it
# for the undivided list: i 1-based list row, j as the rows name the partner (1-based list row, -1..-4, -(4 + k)), in its order, to the bit
function tile_ridgeraft_candidates(eng::HIPEngine)
    n = Ref{Int32}(0); nd = Ref{Int64}(0)
    check(eng, @ccall lib.sz_tile_ridgeraft_candidates(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, Int32(0)::Int32, C_NULL::Ptr{Int64}, C_NULL::Ptr{Int64},
                                                       C_NULL::Ptr{Int32}, C_NULL::Ptr{Float64}, nd::Ptr{Int64})::Cint)
    cap = max(Int(n[]), 1)
    i = Vector{Int64}(undef, cap); j = Vector{Int64}(undef, cap); k = Vector{Int32}(undef, cap); f = Vector{Float64}(undef, cap)
    check(eng, @ccall lib.sz_tile_ridgeraft_candidates(eng.ctx::Ptr{Cvoid}, n::Ptr{Int32}, Int32(cap)::Int32, i::Ptr{Int64}, j::Ptr{Int64},
                                                       k::Ptr{Int32}, f::Ptr{Float64}, nd::Ptr{Int64})::Cint)
    return i[1:n[]] .+ 1, j[1:n[]], Int.(k[1:n[]]), f[1:n[]], Int(nd[])
end

# at a pending stop: the 1-based list number the undivided list gives every local row (owned floes, halo floes, the ghosts of both; n_local rows)
function tile_list_numbers(eng::HIPEngine, n_local::Integer)
    out = Vector{Int64}(undef, max(n_local, 1))
    check(eng, @ccall lib.sz_tile_list_numbers(eng.ctx::Ptr{Cvoid}, out::Ptr{Int64}, length(out)::Int64)::Cint)
    return out[1:n_local] .+ 1
end

# ... and the order key of every local row: the partner column of a downloaded interaction row holds key + 1
function tile_list_keys(eng::HIPEngine, n_local::Integer)
    out = Vector{Int64}(undef, max(n_local, 1))
    check(eng, @ccall lib.sz_tile_list_keys(eng.ctx::Ptr{Cvoid}, out::Ptr{Int64}, length(out)::Int64)::Cint)
    return out[1:n_local]
end

# the second half of the pending step on what the device holds, collectively; the halo rows and ghosts are dropped behind it
function tile_step_finish!(eng::HIPEngine, tstep::Integer, Δt::Integer, coupling_Δt::Integer, flags::Integer)
    check(eng, @ccall lib.sz_tile_step_finish(eng.ctx::Ptr{Cvoid}, Int32(tstep)::Int32, Int32(Δt)::Int32, Int32(coupling_Δt)::Int32, Int32(flags)::Int32)::Cint)
    return
end

# floes that left their tile go to the rank that owns the tile their centroid lies in now (px x py tiles over the domain), with their
# complete state, over the library's channel; collective, between two tile_run! calls.  Returns (floes given away, floes owned now).
function tile_migrate!(eng::HIPEngine, px::Integer, py::Integer)
    sent = Ref{Int64}(0); owned = Ref{Int64}(0)
    check(eng, @ccall lib.sz_tile_migrate(eng.ctx::Ptr{Cvoid}, px::Int32, py::Int32, C_NULL::Ptr{Int32}, sent::Ptr{Int64}, owned::Ptr{Int64})::Cint)
    return Int(sent[]), Int(owned[])
end
# global indices (0-based positions in the undivided floe list) of the floes this rank owns, after tile_migrate! too
function tile_owned(eng::HIPEngine, n_owned::Integer)
    g = Vector{Int64}(undef, max(n_owned, 1))
    check(eng, @ccall lib.sz_tile_owned_gidx(eng.ctx::Ptr{Cvoid}, g::Ptr{Int64}, length(g)::Int64)::Cint)
    return g[1:n_owned]
end

"""
    tile_download_rows!(eng, sub, gidx) -> which

`download_rows!` on a tiled context, by global number (`sz_tile_download_rows`): local, not collective.  `gidx` holds 1-based numbers of the
undivided list in any order, none twice; `sub` is a list of `length(gidx)` floes to receive them (e.g. copies of any floe).  Returns `which`,
the ascending 1-based positions in `gidx` of the floes THIS rank owns; `sub[which[k]]` then holds floe `gidx[which[k]]` -- columns, geometry,
sub-floe points, status and interactions, each value as the rank's full download gives it.  The other entries of `sub` are not touched.  A
host with its own channel gathers `which` and those floes over the ranks, as `TiledWorld.download_rows` does with `all_gather_object`: every
name must be found on exactly one rank.

Written, not run, as `download_rows!` and `splice!` are; the C call underneath is held to the single context's `sz_download_rows` by
`tests/test_splice_tiles_gpu.py`.
"""
function tile_download_rows!(eng::HIPEngine, sub, gidx::AbstractVector{<:Integer})
    n = length(gidx)
    n == 0 && return Int[]
    g0 = Int64.(gidx .- 1)
    which = Vector{Int32}(undef, n); nm = Ref{Int32}(0)
    sizes = Vector{Int64}(undef, 3)
    check(eng, @ccall lib.sz_tile_download_rows(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, g0::Ptr{Int64}, nm::Ptr{Int32}, which::Ptr{Int32}, C_NULL::Ptr{Cvoid},
                                                C_NULL::Ptr{Int32}, C_NULL::Ptr{Float64}, sizes::Ptr{Int64})::Cint)
    m = Int(nm[])
    m == 0 && return Int[]
    mine = Int.(which[1:m]) .+ 1
    got = sub[mine]
    P = pack(got, m)
    resize!(P.vx, sizes[1]); resize!(P.vy, sizes[1]); resize!(P.sx, sizes[2]); resize!(P.sy, sizes[2])
    P.cols.vx = pointer(P.vx); P.cols.vy = pointer(P.vy); P.cols.sx = pointer(P.sx); P.cols.sy = pointer(P.sy)
    off = Vector{Int32}(undef, m + 1); irows = Matrix{Float64}(undef, 7, max(Int(sizes[3]), 1))
    GC.@preserve P got begin
        check(eng, @ccall lib.sz_tile_download_rows(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, g0::Ptr{Int64}, nm::Ptr{Int32}, which::Ptr{Int32}, P.cols::Ref{SzFloeColumns},
                                                    off::Ptr{Int32}, irows::Ptr{Float64}, C_NULL::Ptr{Int64})::Cint)
    end
    unpack_geometry!(got, P); unpack_status!(got, P)
    for k in 1:m
        s = P.sub_off[k]+1:P.sub_off[k+1]
        got.x_subfloe_points[k] = P.sx[s]; got.y_subfloe_points[k] = P.sy[s]
        r = off[k]+1:off[k+1]
        got.interactions[k] = permutedims(irows[:, r]); got.num_inters[k] = length(r)
        got.collision_force[k][1, 1] = P.coll_fx[k]; got.collision_force[k][1, 2] = P.coll_fy[k]
        sub[mine[k]] = got[k]
    end
    return mine
end

"""
    tile_splice!(eng, staged, del, rep, app_owner) -> (N_global, N_owned)

`splice!` on a tiled context, by global number (`sz_tile_splice_floes`): collective, the same arguments on every rank.  `del` and `rep` are
ascending 1-based numbers of the undivided list as it is, none in both; `staged` holds the `length(rep)` replacements, then the appended
floes -- the whole edit, on every rank --, and `app_owner[k]` is the 0-based rank that takes appended floe `k`.  Every rank applies the share
that concerns the floes it owns: no floe data crosses between the ranks.  Afterwards `tile_owned(eng, N_owned)` gives the new numbers of this
rank's floes -- a kept floe's old number minus the deleted floes with a smaller one, appended floe `k` at `N_global_before - length(del) + k`.
Refused on every rank alike, nothing changed (the library's message is thrown): ghosts in the list, a pending ridge / raft step, names that
are unsorted, repeated, out of range or owned twice, an edit that leaves a rank without a floe.

`run_resident!` does not call this.  Written, not run, as `download_rows!` and `splice!` are; the C call underneath is held, bit for bit, to
`sz_splice_floes` of the same edit on the undivided list by `tests/test_splice_tiles_gpu.py`.
"""
function tile_splice!(eng::HIPEngine, staged, del::AbstractVector{<:Integer}, rep::AbstractVector{<:Integer}, app_owner::AbstractVector{<:Integer})
    d0 = Int64.(del .- 1); r0 = Int64.(rep .- 1); own = Int32.(app_owner)
    ng = Ref{Int64}(0); no = Ref{Int64}(0)
    ns = length(staged)
    ns == length(r0) + length(own) || error("tile_splice!: $(ns) staged floes for $(length(r0)) replaced and $(length(own)) appended")
    if ns == 0
        check(eng, @ccall lib.sz_tile_splice_floes(eng.ctx::Ptr{Cvoid}, Int32(length(d0))::Int32, d0::Ptr{Int64}, Int32(0)::Int32, C_NULL::Ptr{Int64}, Int32(0)::Int32,
                                                   C_NULL::Ptr{Int32}, C_NULL::Ptr{Cvoid}, C_NULL::Ptr{Int32}, C_NULL::Ptr{Float64}, ng::Ptr{Int64}, no::Ptr{Int64})::Cint)
    else
        P = pack(staged, ns)
        off, irows = interactions_csr(staged)
        GC.@preserve P staged begin
            check(eng, @ccall lib.sz_tile_splice_floes(eng.ctx::Ptr{Cvoid}, Int32(length(d0))::Int32, d0::Ptr{Int64}, Int32(length(r0))::Int32, r0::Ptr{Int64},
                                                       Int32(length(own))::Int32, own::Ptr{Int32}, P.cols::Ref{SzFloeColumns}, off::Ptr{Int32}, irows::Ptr{Float64},
                                                       ng::Ptr{Int64}, no::Ptr{Int64})::Cint)
        end
    end
    return Int(ng[]), Int(no[])
end

# ... for a Floe{Float32} host, through the _f32 twins on the columns of pack32 (as download_list_rows32 / splice_parents32! above).
# tile_download_rows32: (which, a contiguous copy of sub[which], its Packed32 holding the device's values, inter_off, inter_rows 7 x k)
function tile_download_rows32(eng::HIPEngine, sub::StructArray{<:Floe{Float32}}, gidx::AbstractVector{<:Integer})
    n = length(gidx)
    g0 = Int64.(gidx .- 1)
    which = Vector{Int32}(undef, max(n, 1)); nm = Ref{Int32}(0)
    sizes = Vector{Int64}(undef, 3)
    check(eng, @ccall lib.sz_tile_download_rows_f32(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, g0::Ptr{Int64}, nm::Ptr{Int32}, which::Ptr{Int32}, C_NULL::Ptr{Cvoid},
                                                    C_NULL::Ptr{Int32}, C_NULL::Ptr{Float32}, sizes::Ptr{Int64})::Cint)
    m = Int(nm[])
    mine = Int.(which[1:m]) .+ 1
    got = sub[mine]
    P = pack32(got, m)
    vx = Vector{Float32}(undef, sizes[1]); vy = similar(vx); sx = Vector{Float32}(undef, sizes[2]); sy = similar(sx)
    P.cols.vx = pointer(vx); P.cols.vy = pointer(vy); P.cols.sx = pointer(sx); P.cols.sy = pointer(sy)
    append!(P.keep, Any[vx, vy, sx, sy])
    off = Vector{Int32}(undef, m + 1); irows = Matrix{Float32}(undef, 7, max(Int(sizes[3]), 1))
    GC.@preserve P got begin
        check(eng, @ccall lib.sz_tile_download_rows_f32(eng.ctx::Ptr{Cvoid}, Int32(n)::Int32, g0::Ptr{Int64}, nm::Ptr{Int32}, which::Ptr{Int32},
                                                        P.cols::Ref{SzFloeColumnsF32}, off::Ptr{Int32}, irows::Ptr{Float32}, C_NULL::Ptr{Int64})::Cint)
    end
    return mine, got, P, off, irows
end

# sz_tile_splice_floes_f32 with the whole edit's staged floes packed by pack32; -> (N_global, N_owned)
function tile_splice32!(eng::HIPEngine, staged::StructArray{<:Floe{Float32}}, del::AbstractVector{<:Integer}, rep::AbstractVector{<:Integer},
                        app_owner::AbstractVector{<:Integer})
    isempty(staged) && error("tile_splice32!: nothing replaced or appended (a deletion alone needs no columns: tile_splice!)")
    d0 = Int64.(del .- 1); r0 = Int64.(rep .- 1); own = Int32.(app_owner)
    ng = Ref{Int64}(0); no = Ref{Int64}(0)
    ns = length(staged)
    P = pack32(staged, ns)
    off = Vector{Int32}(undef, ns + 1); off[1] = 0
    for i in 1:ns
        off[i+1] = off[i] + staged.num_inters[i]
    end
    irows = Matrix{Float32}(undef, 7, max(Int(off[end]), 1))
    for i in 1:ns, k in 1:staged.num_inters[i]
        irows[:, off[i]+k] .= @view staged.interactions[i][k, :]
    end
    GC.@preserve P staged begin
        check(eng, @ccall lib.sz_tile_splice_floes_f32(eng.ctx::Ptr{Cvoid}, Int32(length(d0))::Int32, d0::Ptr{Int64}, Int32(length(r0))::Int32, r0::Ptr{Int64},
                                                       Int32(length(own))::Int32, own::Ptr{Int32}, P.cols::Ref{SzFloeColumnsF32}, off::Ptr{Int32},
                                                       irows::Ptr{Float32}, ng::Ptr{Int64}, no::Ptr{Int64})::Cint)
    end
    return Int(ng[]), Int(no[])
end

# ------------------------------------------------------------------------------------------------ output frames on the device
# include/subzero_hip.h, "output frames on the device": sz_step cuts before the output steps of registered writers and records what they
# would take into device memory; drain_frames! writes the frames through the writers' own files afterwards.
# The bits of sz_set_floe_output's mask, bit 0 first (sz_debug_frame_bits)
const FRAME_BITS = (:cx, :cy, :rmax, :area, :height, :mass, :moment, :alpha, :u, :v, :xi, :p_dxdt, :p_dydt, :p_dalphadt, :p_dudt, :p_dvdt,
                    :p_dxidt, :fxOA, :fyOA, :trqOA, :hflx_factor, :overarea, :coll_fx, :coll_fy, :coll_trq, :stress_accum, :stress_instant,
                    :strain, :id, :ghost_id, :status, :rings, :ghost_links)
frame_mask(groups) = reduce(|, (UInt64(1) << (findfirst(==(g), FRAME_BITS) - 1) for g in groups); init = UInt64(0))
# FloeOutputWriter outputs a frame's columns give as they are, and the column groups each needs.  The other fields of Floe: the tables below
const FRAME_OUTPUTS = Dict{Symbol, Vector{Symbol}}(
    :centroid => [:cx, :cy], :coords => [:rings], :height => [:height], :area => [:area], :mass => [:mass], :rmax => [:rmax],
    :moment => [:moment], :α => [:alpha], :u => [:u], :v => [:v], :ξ => [:xi], :id => [:id], :ghost_id => [:ghost_id],
    :ghosts => [:ghost_links], :fxOA => [:fxOA], :fyOA => [:fyOA], :trqOA => [:trqOA], :hflx_factor => [:hflx_factor],
    :overarea => [:overarea], :collision_force => [:coll_fx, :coll_fy], :collision_trq => [:coll_trq], :stress_accum => [:stress_accum],
    :stress_instant => [:stress_instant], :strain => [:strain], :p_dxdt => [:p_dxdt], :p_dydt => [:p_dydt], :p_dudt => [:p_dudt],
    :p_dvdt => [:p_dvdt], :p_dξdt => [:p_dxidt], :p_dαdt => [:p_dalphadt])
# The lists of sz_set_floe_output_lists, bit 0 first (SZ_FRAME_INTERACTIONS, SZ_FRAME_SUBPOINTS)
const FRAME_LISTS = (:interactions, :subpoints)
# Outputs a frame serves through more than a copy of a column: output => (column groups, lists)
#   :interactions, :num_inters   the interactions section; the matrix written is rows 1:num_inters (the reference's file can also hold stale
#                                rows past num_inters -- the matrix only grows, collisions.jl:290-296 -- which no reader may use)
#   :status                      Status(tag, Int[]): fuse_idx is non-empty only on a row tagged `fuse`, and a batch that honours tags never
#                                begins a step with one (an error if a frame shows one)
#   :poly                        Subzero.make_polygon of the recorded ring
const FRAME_DERIVED_OUTPUTS = Dict{Symbol, Tuple{Vector{Symbol}, Vector{Symbol}}}(
    :interactions => (Symbol[], [:interactions]), :num_inters => (Symbol[], [:interactions]),
    :status => ([:status], Symbol[]), :poly => ([:rings], Symbol[]))
# Outputs taken from the HOST's own floes, matched by the recorded id (each needs the :id group): nothing in a batch changes them, a ghost
# carries its parent's id, and matching by id survives removals on the device.  The sub-floe points are deliberately not pulled through the
# frame's section here -- about 16 MB per frame at 10 000 floes of data that is constant between host edits; the section is for hosts that
# keep no floe list, and for restarts.  parent_ids: emptied after the first frame written for an output step, as write_floe_data! does
# (output.jl:570).
const FRAME_HOST_OUTPUTS = (:angles, :damage, :parent_ids, :x_subfloe_points, :y_subfloe_points)
frame_covers(w) = all(o -> haskey(FRAME_OUTPUTS, o) || haskey(FRAME_DERIVED_OUTPUTS, o) || o in FRAME_HOST_OUTPUTS, w.outputs)
# the column groups and the lists word a writer's outputs need
function frame_needs(outputs)
    groups, lists = Symbol[], UInt32(0)
    for o in outputs
        if haskey(FRAME_OUTPUTS, o)
            append!(groups, FRAME_OUTPUTS[o])
        elseif haskey(FRAME_DERIVED_OUTPUTS, o)
            g, l = FRAME_DERIVED_OUTPUTS[o]
            append!(groups, g)
            for name in l
                lists |= UInt32(1) << (findfirst(==(name), FRAME_LISTS) - 1)
            end
        else
            push!(groups, :id)
        end
    end
    isempty(groups) && push!(groups, :id)          # (a mask selects at least one group)
    return frame_mask(groups), lists
end
frame_lists(w) = frame_needs(w.outputs)[2]
const EUL_CODES = Dict(name => Int32(k - 1) for (k, name) in enumerate(
    (:u_grid, :v_grid, :dudt_grid, :dvdt_grid, :overarea_grid, :mass_grid, :area_grid, :height_grid, :si_frac_grid, :stress_xx_grid,
     :stress_yx_grid, :stress_xy_grid, :stress_yy_grid, :stress_eig_grid, :strain_ux_grid, :strain_vx_grid, :strain_uy_grid, :strain_vy_grid)))

"""
    set_floe_output!(eng, sim, i; arena_bytes = 1 << 28) -> Bool

Register `sim.writers.floewriters[i]` with the device recorder (at most 4): its Δtout, the column groups and the lists its outputs need
(`frame_needs`; the `id` group where an output is served from the host's floes).  `false`, and nothing registered, when the writer asks for
an output a frame does not serve.
"""
function set_floe_output!(eng::HIPEngine, sim, i::Integer; arena_bytes::Integer = 1 << 28)
    w = sim.writers.floewriters[i]
    (frame_covers(w) && length(eng.rec_floe) < 4) || return false
    mask, lists = frame_needs(w.outputs)
    check(eng, @ccall lib.sz_set_floe_output(eng.ctx::Ptr{Cvoid}, Int32(length(eng.rec_floe))::Int32, Int32(w.Δtout)::Int32, mask::UInt64,
                                             Int64(arena_bytes)::Int64)::Cint)
    lists != 0 && check(eng, @ccall lib.sz_set_floe_output_lists(eng.ctx::Ptr{Cvoid}, Int32(length(eng.rec_floe))::Int32, lists::UInt32)::Cint)
    push!(eng.rec_floe, (Int(i), mask))
    return true
end

"""
    set_grid_output!(eng, sim, i; max_frames = 64) -> Bool

Register `sim.writers.gridwriters[i]` with the device recorder (at most 4): Δtout, grid lines and outputs.
"""
function set_grid_output!(eng::HIPEngine, sim, i::Integer; max_frames::Integer = 64)
    w = sim.writers.gridwriters[i]
    length(eng.rec_grid) < 4 || return false
    xg, yg = collect(Float64, w.xg), collect(Float64, w.yg)
    codes = Int32[EUL_CODES[o] for o in w.outputs]
    check(eng, @ccall lib.sz_set_grid_output(eng.ctx::Ptr{Cvoid}, Int32(length(eng.rec_grid))::Int32, Int32(w.Δtout)::Int32,
                                             Int32(length(xg) - 1)::Int32, Int32(length(yg) - 1)::Int32, xg::Ptr{Float64}, yg::Ptr{Float64},
                                             Int32(length(codes))::Int32, codes::Ptr{Int32}, Int32(max_frames)::Int32)::Cint)
    push!(eng.rec_grid, Int(i))
    return true
end

tensor(t, i) = [t[4i-3] t[4i-2]; t[4i-1] t[4i]]          # 11, 12, 21, 22
# one output of a FloeOutputWriter from the columns of a frame, as StructArrays.component(floes, output) would give it
function frame_component(o::Symbol, c::Dict{Symbol, Vector}, M::Int)
    if o === :interactions          # rows 1:num_inters of every floe (c[:inter_rows][1]: 7 x R, a row of the matrix per column)
        rows = c[:inter_rows][1]
        return [permutedims(rows[:, c[:inter_off][i]+1:c[:inter_off][i+1]]) for i in 1:M]
    end
    o === :num_inters && return [Int(c[:inter_off][i+1] - c[:inter_off][i]) for i in 1:M]
    if o === :status          # (tags: active = 1, remove = 2, fuse = 3 -- SZ_ACTIVE .. SZ_FUSE, floe.jl:8-12)
        any(==(Int32(3)), c[:status]) && error("a frame began a step with a floe tagged fuse: its fuse_idx is not recorded")
        return [Subzero.Status(Subzero.StatusTag(Int(t)), Int[]) for t in c[:status]]
    end
    o === :poly && return [Subzero.make_polygon([[[c[:vx][k], c[:vy][k]] for k in c[:vert_off][i]+1:c[:vert_off][i+1]]]) for i in 1:M]
    o === :centroid && return [[c[:cx][i], c[:cy][i]] for i in 1:M]
    o === :coords && return [[[[c[:vx][k], c[:vy][k]] for k in c[:vert_off][i]+1:c[:vert_off][i+1]]] for i in 1:M]
    o === :ghosts && return [Int[c[:ghost_idx][k] + 1 for k in c[:ghost_off][i]+1:c[:ghost_off][i+1]] for i in 1:M]
    o === :collision_force && return [[c[:coll_fx][i] c[:coll_fy][i]] for i in 1:M]
    o in (:stress_accum, :stress_instant, :strain) && return [tensor(c[o], i) for i in 1:M]
    o in (:id, :ghost_id) && return Int.(c[o])
    return c[FRAME_OUTPUTS[o][1]]
end

"""
    drain_frames!(eng, sim)

Write every frame the device holds through the writers' own files -- `write_field` under `output/tstep` for a FloeOutputWriter, the NetCDF
slice `istep = div(tstep, Δtout) + 1` for a GridOutputWriter (output.jl:558-605) -- and clear them.  Returns whether the last batch ended on
a frame that found no room.
"""
function drain_frames!(eng::HIPEngine, sim)
    nf, ng, full = zeros(Int32, 4), zeros(Int32, 4), Ref{Int32}(0)
    check(eng, @ccall lib.sz_output_frames(eng.ctx::Ptr{Cvoid}, nf::Ptr{Int32}, ng::Ptr{Int32}, full::Ptr{Int32})::Cint)
    emptied = Set{Int}()          # output steps whose parent_ids have been written once (output.jl:570)
    for (slot, (i, mask)) in enumerate(eng.rec_floe), k in 0:nf[slot]-1
        w = sim.writers.floewriters[i]
        lists = frame_lists(w)
        info = [Ref{Int64}(0) for _ in 1:5]
        check(eng, @ccall lib.sz_floe_frame_info(eng.ctx::Ptr{Cvoid}, Int32(slot - 1)::Int32, Int32(k)::Int32, info[1]::Ptr{Int64},
                                                 info[2]::Ptr{Int64}, info[3]::Ptr{Int64}, info[4]::Ptr{Int64}, info[5]::Ptr{Int64})::Cint)
        tstep, M, _, V, G = (Int(r[]) for r in info)
        cols, c = SzFloeColumns(), Dict{Symbol, Vector}()
        for (b, g) in enumerate(FRAME_BITS)
            (mask >> (b - 1)) & 1 == 1 || continue
            if g === :rings
                c[:vert_off], c[:vx], c[:vy] = zeros(Int32, M + 1), zeros(Float64, max(V, 1)), zeros(Float64, max(V, 1))
            elseif g === :ghost_links
                c[:ghost_off], c[:ghost_idx] = zeros(Int32, M + 1), zeros(Int32, max(G, 1))
            elseif g === :status
                c[g] = zeros(Int32, M)
            elseif g in (:id, :ghost_id)
                c[g] = zeros(Int64, M)
            else
                c[g] = zeros(Float64, (b > 25 ? 4 : 1) * M)
            end
        end
        GC.@preserve c begin
            for (name, v) in c
                setfield!(cols, name, pointer(v))
            end
            check(eng, @ccall lib.sz_download_floe_frame(eng.ctx::Ptr{Cvoid}, Int32(slot - 1)::Int32, Int32(k)::Int32,
                                                         cols::Ref{SzFloeColumns})::Cint)
        end
        if lists & 1 != 0
            nr, ns = Ref{Int64}(0), Ref{Int64}(0)
            check(eng, @ccall lib.sz_floe_frame_lists_info(eng.ctx::Ptr{Cvoid}, Int32(slot - 1)::Int32, Int32(k)::Int32, nr::Ptr{Int64},
                                                           ns::Ptr{Int64})::Cint)
            ioff, irows = zeros(Int32, M + 1), zeros(Float64, 7, max(Int(nr[]), 1))
            check(eng, @ccall lib.sz_download_floe_frame_interactions(eng.ctx::Ptr{Cvoid}, Int32(slot - 1)::Int32, Int32(k)::Int32,
                                                                      ioff::Ptr{Int32}, irows::Ptr{Float64})::Cint)
            c[:inter_off], c[:inter_rows] = ioff, [irows]
        end
        # outputs of the host's own floes, by the recorded id (a ghost: its parent's)
        floes = sim.model.floes
        row_of = Dict(id => r for (r, id) in enumerate(floes.id))
        host_rows = any(in(FRAME_HOST_OUTPUTS), w.outputs) ? [row_of[Int(id)] for id in c[:id]] : Int[]
        Subzero.jldopen(w.filepath, "a+") do file
            for o in w.outputs
                if o in FRAME_HOST_OUTPUTS
                    v = o === :parent_ids && tstep in emptied ? [Int[] for _ in host_rows] : [getproperty(floes, o)[r] for r in host_rows]
                    Subzero.write_field(file, string(o, "/", tstep), v)
                else
                    Subzero.write_field(file, string(o, "/", tstep), frame_component(o, c, M))
                end
            end
        end
        :parent_ids in w.outputs && push!(emptied, tstep)
    end
    for (slot, i) in enumerate(eng.rec_grid), k in 0:ng[slot]-1
        w = sim.writers.gridwriters[i]
        nx, ny, nout = length(w.xg) - 1, length(w.yg) - 1, length(w.outputs)
        tstep, data = Ref{Int32}(0), Vector{Float64}(undef, nout * nx * ny)
        check(eng, @ccall lib.sz_download_grid_frame(eng.ctx::Ptr{Cvoid}, Int32(slot - 1)::Int32, Int32(k)::Int32, tstep::Ptr{Int32},
                                                     data::Ptr{Float64})::Cint)
        d = permutedims(reshape(data, ny, nx, nout), (2, 1, 3))          # data[k][ix][iy], row-major -> [ix, iy, k]
        istep = div(Int(tstep[]), w.Δtout) + 1
        ds = Subzero.NCDataset(w.filepath, "a")
        for j in eachindex(w.outputs)
            ds[string(w.outputs[j])][istep, :, :] = d[:, :, j]
        end
        close(ds)
    end
    check(eng, @ccall lib.sz_clear_frames(eng.ctx::Ptr{Cvoid})::Cint)
    return full[] != 0
end

# write_data! (output.jl:478-499) for the writers the recorder does not serve: the registered ones get that step's frame from the device
function write_host_data!(sim, eng::HIPEngine, tstep, start_tstep)
    tstep == start_tstep && Subzero.write_init_state_data!(sim)
    Subzero.write_checkpoint_data!(sim, tstep)
    fw, gw = sim.writers.floewriters, sim.writers.gridwriters
    Subzero.write_floe_data!(fw[[k for k in eachindex(fw) if !(k in first.(eng.rec_floe))]], sim.model.floes, tstep)
    Subzero.write_grid_data!(gw[[k for k in eachindex(gw) if !(k in eng.rec_grid)]], sim.model.floes, sim.model.domain.topography, tstep)
    return
end

# the writers the host still serves: with device_output the registered ones leave the list
function writer_periods(w, eng = nothing)
    on_device(ws, idx) = eng === nothing ? ws : [x for (k, x) in enumerate(ws) if !(k in idx)]
    fl = on_device(w.floewriters, eng === nothing ? () : first.(eng.rec_floe))
    gr = on_device(w.gridwriters, eng === nothing ? () : eng.rec_grid)
    return Int[x.Δtout for ws in (fl, gr, w.checkpointwriters) for x in ws]
end
output_due(w, tstep, start, eng = nothing) = tstep == start || any(p -> mod(tstep, p) == 0, writer_periods(w, eng))
function steps_to_next_output(w, tstep, start, eng = nothing)
    ps = writer_periods(w, eng)
    isempty(ps) && return typemax(Int32) ÷ 2
    return minimum(p - mod(tstep, p) for p in ps)
end


# ------------------------------------------------------------------------------------------------ Float32 hosts
# Floe{FT} is generic (floe.jl:24) although only Float64 is tested and supported (documentation.md:25).  The library's `_f32` entry points
# take the columns of a Floe{Float32} field as they lie, widen them on the way in, compute as for a Float64 host and round on the way out.
# The column traffic of such a host: `upload32!` / `download32!` below (the process-mode boundary); the overloads of the three hot calls
# above stay Float64 methods -- for a Float32 simulation they are the same bodies with these two in place of `upload!` / `download!`,
# `sz_set_fields_f32` for the lattices and `sz_download_interactions_f32` for floe.interactions.
struct Packed32
    cols::SzFloeColumnsF32
    keep::Vector{Any}                     # every flattened vector the pointers point into
    status::Vector{Int32}
end

function pack32(floes::StructArray{<:Floe{Float32}}, n_parents::Integer)
    M = length(floes)
    cx = Float32[c[1] for c in floes.centroid]; cy = Float32[c[2] for c in floes.centroid]
    coll_fx = Float32[f[1, 1] for f in floes.collision_force]; coll_fy = Float32[f[1, 2] for f in floes.collision_force]
    sa = Vector{Float32}(undef, 4M); si = similar(sa); st = similar(sa)
    for i in 1:M
        sa[4i-3:4i] .= tensor4(floes.stress_accum[i]); si[4i-3:4i] .= tensor4(floes.stress_instant[i])
        st[4i-3:4i] .= tensor4(floes.strain[i])
    end
    status = Int32[Int32(s.tag) for s in floes.status]
    vert_off = Vector{Int32}(undef, M + 1); vert_off[1] = 0
    vx = Float32[]; vy = Float32[]
    for i in 1:M
        for pt in GI.getpoint(GI.getexterior(floes.poly[i]))
            push!(vx, GI.x(pt)); push!(vy, GI.y(pt))
        end
        vert_off[i+1] = length(vx)
    end
    sub_off = Vector{Int32}(undef, n_parents + 1); sub_off[1] = 0
    sx = Float32[]; sy = Float32[]
    for i in 1:n_parents
        append!(sx, floes.x_subfloe_points[i]); append!(sy, floes.y_subfloe_points[i])
        sub_off[i+1] = length(sx)
    end
    id = Vector{Int64}(floes.id); ghost_id = Vector{Int64}(floes.ghost_id)
    c = SzFloeColumnsF32()
    c.cx = pointer(cx); c.cy = pointer(cy)
    c.rmax = pointer(floes.rmax); c.area = pointer(floes.area); c.height = pointer(floes.height)
    c.mass = pointer(floes.mass); c.moment = pointer(floes.moment); c.alpha = pointer(floes.α)
    c.u = pointer(floes.u); c.v = pointer(floes.v); c.xi = pointer(floes.ξ)
    c.p_dxdt = pointer(floes.p_dxdt); c.p_dydt = pointer(floes.p_dydt); c.p_dalphadt = pointer(floes.p_dαdt)
    c.p_dudt = pointer(floes.p_dudt); c.p_dvdt = pointer(floes.p_dvdt); c.p_dxidt = pointer(floes.p_dξdt)
    c.fxOA = pointer(floes.fxOA); c.fyOA = pointer(floes.fyOA); c.trqOA = pointer(floes.trqOA)
    c.hflx_factor = pointer(floes.hflx_factor); c.overarea = pointer(floes.overarea)
    c.coll_fx = pointer(coll_fx); c.coll_fy = pointer(coll_fy); c.coll_trq = pointer(floes.collision_trq)
    c.stress_accum = pointer(sa); c.stress_instant = pointer(si); c.strain = pointer(st)
    c.id = pointer(id); c.ghost_id = pointer(ghost_id); c.status = pointer(status)
    c.vert_off = pointer(vert_off); c.vx = pointer(vx); c.vy = pointer(vy)
    c.sub_off = pointer(sub_off); c.sx = pointer(sx); c.sy = pointer(sy)
    return Packed32(c, Any[cx, cy, coll_fx, coll_fy, sa, si, st, vert_off, vx, vy, sub_off, sx, sy, id, ghost_id], status)
end

function upload32!(eng::HIPEngine, floes::StructArray{<:Floe{Float32}}, n_parents)
    P = pack32(floes, n_parents)
    GC.@preserve P floes begin
        check(eng, @ccall lib.sz_upload_floes_f32(eng.ctx::Ptr{Cvoid}, length(floes)::Int64, n_parents::Int64,
                                                  P.cols::Ref{SzFloeColumnsF32})::Cint)
    end
    return P
end

function download32!(eng::HIPEngine, floes::StructArray{<:Floe{Float32}}, P::Packed32)
    GC.@preserve P floes begin
        check(eng, @ccall lib.sz_download_floes_f32(eng.ctx::Ptr{Cvoid}, P.cols::Ref{SzFloeColumnsF32})::Cint)
    end
    return
end

end # module
