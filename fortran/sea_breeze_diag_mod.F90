!===============================================================================
! sea_breeze_diag_mod -- drop-in Fortran host module for the MI355X implementation.
!
! Same module name, same four public routines and the same dummy-argument order as the
! reference's generic module (ref: generic/sea_breeze_diag.f90:19, :55-56, :273, :375,
! :457), so a host model keeps its `use sea_breeze_diag_mod` / `call seabreeze_diag(...)`
! lines (ref: generic/dummy_model.f90:28,41,52).  Every routine is a thin ISO_C_BINDING
! shim over libseabreeze_hip.so (include/seabreeze_hip.h): descriptor in, contiguous
! buffers + extents out.  No arithmetic of the diagnostic lives here.
!
! Working precision follows the compile flag like the reference:
!   amdflang ...                              -> REAL = 4 bytes -> sb_*_f32
!   amdflang -fdefault-real-8 -DSB_REAL8 ...  -> REAL = 8 bytes -> sb_*_f64
!
! Beyond the reference's four routines (same names, same dummies) the module offers what a host
! model needs to use more than one GPU or to keep its fields on the device:
!   band_seabreeze_diag      one step of a latitude band (host arrays, ghost cells of width h): the
!                            sigma statistics are reduced over all bands and theta's ghost rows are
!                            exchanged over RCCL inside the call (sb_context_mod::sb_comm_init first)
!   seabreeze_diag_dev,      the same two calls with every array a device pointer (type(c_ptr) from
!   band_seabreeze_diag_dev  sb_context_mod::sb_dev_alloc): enqueue only, nothing crosses PCIe
!
! Errors: the reference's generic routines have no error channel; a non-zero status from
! the library ends the run with `error stop` and the library's message.  The UM hook's
! `error` out-argument (ref: UM/vn10.7/sea_breeze_diag.F90:102) is available through
! seabreeze_diag_status.
!
! Array conventions accepted by seabreeze_diag (all assumed-shape, as in the reference):
!   p, u, v                      (nx, ny, nz)
!   windspeed, winddir, thc, sb_con   (nx, ny)
!   theta, mask, z, sigma        (nx, ny)            -> single global domain: latitude is
!                                                       clamped, longitude periodic
!                                (nx+2h, ny+2h)      -> ghost cells of width h all round
!                                                       (what swap_bounds fills); raw reads
!===============================================================================
module sea_breeze_diag_mod
  use iso_c_binding
  use sb_context_mod, only : ctx => sb_ctx, ensure_ctx => sb_ensure_ctx, fail => sb_fail, sb_release_ctx
  implicit none
  private
  public :: seabreeze_diag, seabreeze_diag_status, get_edges, get_dist, sigmoid, sb_shutdown
  public :: band_seabreeze_diag, seabreeze_diag_dev, band_seabreeze_diag_dev
  public :: seabreeze_diag_um, SB_UM_THETA_TO_T0, SB_UM_LEVEL_WALK
  public :: get_edges_um, get_dist_um, get_dist_um_win
  public :: tile_get_edges_um, tile_get_dist_um, SB_TILE_WEST, SB_TILE_EAST, SB_TILE_SOUTH, SB_TILE_NORTH
  public :: band_get_edges, band_get_dist, band_get_edges_dev, band_get_dist_dev
  public :: band_coast_open, band_ice_dev, band_ice_report, band_coast_close
  public :: um_coast_open, um_ice, um_ice_dev, um_ice_report, um_coast_close
  public :: um_tile_coast_open, um_tile_ice, um_tile_ice_dev, um_tile_ice_report, um_tile_coast_close
  public :: search_radius, band_search_radius
  integer, parameter :: SB_UM_THETA_TO_T0 = 1, SB_UM_LEVEL_WALK = 2

#ifdef SB_REAL8
  integer, parameter :: rk = c_double
#define SB_SEABREEZE_DIAG "sb_seabreeze_diag_f64"
#define SB_SIGMOID        "sb_sigmoid_f64"
#define SB_GET_EDGES      "sb_get_edges_f64"
#define SB_GET_DIST       "sb_get_dist_f64"
#define SB_BAND_DIAG      "sb_band_seabreeze_diag_f64"
#define SB_DIAG_DEV       "sb_seabreeze_diag_f64_dev"
#define SB_BAND_DIAG_DEV  "sb_band_seabreeze_diag_f64_dev"
#define SB_DIAG_UM        "sb_seabreeze_diag_um_f64"
#define SB_GET_EDGES_UM   "sb_get_edges_um_f64"
#define SB_GET_DIST_UM    "sb_get_dist_um_f64"
#define SB_GET_DIST_UM_WIN "sb_get_dist_um_win_f64"
#define SB_TILE_GET_EDGES_UM "sb_tile_get_edges_um_f64"
#define SB_TILE_GET_DIST_UM  "sb_tile_get_dist_um_f64"
#define SB_BAND_GET_EDGES "sb_band_get_edges_f64"
#define SB_BAND_GET_DIST  "sb_band_get_dist_f64"
#define SB_BAND_GET_EDGES_DEV "sb_band_get_edges_f64_dev"
#define SB_BAND_GET_DIST_DEV  "sb_band_get_dist_f64_dev"
#define SB_BAND_COAST_OPEN    "sb_band_coast_open_f64"
#define SB_BAND_ICE_DEV       "sb_band_ice_f64_dev"
#define SB_UM_COAST_OPEN      "sb_um_coast_open_f64"
#define SB_UM_ICE             "sb_um_ice_f64"
#define SB_UM_ICE_DEV         "sb_um_ice_f64_dev"
#define SB_UM_TILE_COAST_OPEN "sb_um_tile_coast_open_f64"
#define SB_UM_TILE_ICE        "sb_um_tile_ice_f64"
#define SB_UM_TILE_ICE_DEV    "sb_um_tile_ice_f64_dev"
#define SB_SEARCH_RADIUS      "sb_search_radius_f64"
#define SB_BAND_SEARCH_RADIUS "sb_band_search_radius_f64"
#else
  integer, parameter :: rk = c_float
#define SB_SEABREEZE_DIAG "sb_seabreeze_diag_f32"
#define SB_SIGMOID        "sb_sigmoid_f32"
#define SB_GET_EDGES      "sb_get_edges_f32"
#define SB_GET_DIST       "sb_get_dist_f32"
#define SB_BAND_DIAG      "sb_band_seabreeze_diag_f32"
#define SB_DIAG_DEV       "sb_seabreeze_diag_f32_dev"
#define SB_BAND_DIAG_DEV  "sb_band_seabreeze_diag_f32_dev"
#define SB_DIAG_UM        "sb_seabreeze_diag_um_f32"
#define SB_GET_EDGES_UM   "sb_get_edges_um_f32"
#define SB_GET_DIST_UM    "sb_get_dist_um_f32"
#define SB_GET_DIST_UM_WIN "sb_get_dist_um_win_f32"
#define SB_TILE_GET_EDGES_UM "sb_tile_get_edges_um_f32"
#define SB_TILE_GET_DIST_UM  "sb_tile_get_dist_um_f32"
#define SB_BAND_GET_EDGES "sb_band_get_edges_f32"
#define SB_BAND_GET_DIST  "sb_band_get_dist_f32"
#define SB_BAND_GET_EDGES_DEV "sb_band_get_edges_f32_dev"
#define SB_BAND_GET_DIST_DEV  "sb_band_get_dist_f32_dev"
#define SB_BAND_COAST_OPEN    "sb_band_coast_open_f32"
#define SB_BAND_ICE_DEV       "sb_band_ice_f32_dev"
#define SB_UM_COAST_OPEN      "sb_um_coast_open_f32"
#define SB_UM_ICE             "sb_um_ice_f32"
#define SB_UM_ICE_DEV         "sb_um_ice_f32_dev"
#define SB_UM_TILE_COAST_OPEN "sb_um_tile_coast_open_f32"
#define SB_UM_TILE_ICE        "sb_um_tile_ice_f32"
#define SB_UM_TILE_ICE_DEV    "sb_um_tile_ice_f32_dev"
#define SB_SEARCH_RADIUS      "sb_search_radius_f32"
#define SB_BAND_SEARCH_RADIUS "sb_band_search_radius_f32"
#endif

  integer(c_int), parameter :: SB_BND_GLOBAL = 1, SB_BND_HALO = 2
  ! the sides of a tile that are the domain's edge (tile_get_edges_um, tile_get_dist_um; include/seabreeze_hip.h: SB_TILE_*)
  integer, parameter :: SB_TILE_WEST = 1, SB_TILE_EAST = 2, SB_TILE_SOUTH = 4, SB_TILE_NORTH = 8
  integer(c_int), save :: um_shape(4) = 0     ! nx, ny, halo_i, halo_j of the open UM coast (um_coast_open)
  integer(c_int), save :: um_tile_shape(4) = 0   ! the same of the open UM tile coast (um_tile_coast_open)

  interface band_get_dist       ! (maxdist as a real or as the integer literal, like get_dist)
    module procedure band_get_dist_r
    module procedure band_get_dist_i
  end interface

  interface get_dist            ! the reference's caller passes the integer literal 180 for
    module procedure get_dist_r ! maxdist (ref: generic/dummy_model.f90:33); accept both
    module procedure get_dist_i
  end interface

  interface
    integer(c_int) function c_seabreeze_diag(ctx, timestep, tn, nx, ny, nz, halo, bnd, p, u, v, theta, mask, &
        z, sigma, ws, wd, thc, sb_con, tun) bind(C, name=SB_SEABREEZE_DIAG)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx, tun
      real(rk), value :: timestep
      integer(c_int), value :: tn, nx, ny, nz, halo, bnd
      real(rk), intent(in) :: p(*), u(*), v(*), theta(*), mask(*), z(*), sigma(*)
      real(rk), intent(inout) :: ws(*), wd(*), thc(*), sb_con(*)
    end function
    integer(c_int) function c_diag_um(ctx, timestep, tn, nx, ny, nz, halo_s, halo_l, p, u, v, theta, z, sigma, mask, &
        ws, wd, thc, sb_con, flags, error) bind(C, name=SB_DIAG_UM)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      real(rk), value :: timestep
      integer(c_int), value :: tn, nx, ny, nz, halo_s, halo_l, flags
      real(rk), intent(in) :: p(*), u(*), v(*), z(*), sigma(*), mask(*)
      real(rk), intent(inout) :: theta(*), ws(*), wd(*), thc(*), sb_con(*)
      integer(c_int), intent(out) :: error
    end function c_diag_um
    integer(c_int) function c_band_diag(ctx, timestep, tn, nx, ny, nz, halo, p, u, v, theta, mask, &
        z, sigma, ws, wd, thc, sb_con, tun) bind(C, name=SB_BAND_DIAG)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx, tun
      real(rk), value :: timestep
      integer(c_int), value :: tn, nx, ny, nz, halo
      real(rk), intent(in) :: p(*), u(*), v(*), mask(*), z(*), sigma(*)
      real(rk), intent(inout) :: theta(*), ws(*), wd(*), thc(*), sb_con(*)
    end function
    integer(c_int) function c_diag_dev(ctx, timestep, tn, nx, ny, nz, halo, bnd, p, u, v, theta, mask, &
        z, sigma, ws, wd, thc, sb_con, tun, stream) bind(C, name=SB_DIAG_DEV)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx, tun, stream, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con
      real(rk), value :: timestep
      integer(c_int), value :: tn, nx, ny, nz, halo, bnd
    end function
    integer(c_int) function c_band_diag_dev(ctx, timestep, tn, nx, ny, nz, halo, p, u, v, theta, mask, &
        z, sigma, ws, wd, thc, sb_con, tun, stream) bind(C, name=SB_BAND_DIAG_DEV)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx, tun, stream, p, u, v, theta, mask, z, sigma, ws, wd, thc, sb_con
      real(rk), value :: timestep
      integer(c_int), value :: tn, nx, ny, nz, halo
    end function
    integer(c_int) function c_sigmoid(ctx, nx, ny, ary, sm) bind(C, name=SB_SIGMOID)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny
      real(rk), intent(in) :: ary(*)
      real(rk), intent(out) :: sm(*)
    end function
    integer(c_int) function c_get_edges(ctx, nx, ny, lsm, ci, rule, bnd, coast) bind(C, name=SB_GET_EDGES)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, rule, bnd
      real(rk), intent(in) :: lsm(*), ci(*)
      real(rk), intent(out) :: coast(*)
    end function
    integer(c_int) function c_get_dist(ctx, nx, ny, coast, mask, lon, lat, maxdist, kwin, cdist) &
        bind(C, name=SB_GET_DIST)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, kwin
      real(rk), value :: maxdist
      real(rk), intent(in) :: coast(*), mask(*), lon(*), lat(*)
      real(rk), intent(out) :: cdist(*)
    end function
    integer(c_int) function c_get_edges_um(ctx, nx, ny, hi, hj, lf, ci, coast) bind(C, name=SB_GET_EDGES_UM)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, hi, hj
      real(rk), intent(in) :: lf(*), ci(*)
      real(rk), intent(inout) :: coast(*)
    end function
    integer(c_int) function c_get_dist_um(ctx, nx, ny, hi, hj, coast, lf, tlat, tlon, maxdist, cdist) &
        bind(C, name=SB_GET_DIST_UM)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, hi, hj
      real(rk), value :: maxdist
      real(rk), intent(in) :: coast(*), lf(*), tlat(*), tlon(*)
      real(rk), intent(inout) :: cdist(*)
    end function
    integer(c_int) function c_get_dist_um_win(ctx, nx, ny, hi, hj, wi, wj, coast, lf, tlat, tlon, maxdist, cdist) &
        bind(C, name=SB_GET_DIST_UM_WIN)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, hi, hj, wi, wj
      real(rk), value :: maxdist
      real(rk), intent(in) :: coast(*), lf(*), tlat(*), tlon(*)
      real(rk), intent(inout) :: cdist(*)
    end function
    integer(c_int) function c_tile_get_edges_um(ctx, nx, ny, hi, hj, ei, ej, sides, lf, ci, coast) &
        bind(C, name=SB_TILE_GET_EDGES_UM)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, hi, hj, ei, ej, sides
      real(rk), intent(in) :: lf(*), ci(*)
      real(rk), intent(inout) :: coast(*)
    end function
    integer(c_int) function c_tile_get_dist_um(ctx, nx, ny, hi, hj, wi, wj, sides, coast, lf, tlat, tlon, maxdist, cdist) &
        bind(C, name=SB_TILE_GET_DIST_UM)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, hi, hj, wi, wj, sides
      real(rk), value :: maxdist
      real(rk), intent(in) :: coast(*), lf(*), tlat(*), tlon(*)
      real(rk), intent(inout) :: cdist(*)
    end function
    integer(c_int) function c_band_get_edges(ctx, nx, ny, halo, south, north, lsm, ci, rule, coast) &
        bind(C, name=SB_BAND_GET_EDGES)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, halo, south, north, rule
      real(rk), intent(in) :: lsm(*), ci(*)
      real(rk), intent(inout) :: coast(*)
    end function
    integer(c_int) function c_band_get_dist(ctx, nx, ny, halo, south, north, coast, mask, lon, lat, maxdist, kwin, cdist) &
        bind(C, name=SB_BAND_GET_DIST)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, halo, south, north, kwin
      real(rk), value :: maxdist
      real(rk), intent(in) :: coast(*), mask(*), lon(*), lat(*)
      real(rk), intent(inout) :: cdist(*)
    end function
    integer(c_int) function c_band_get_edges_dev(ctx, nx, ny, halo, south, north, lsm, ci, rule, coast, stream) &
        bind(C, name=SB_BAND_GET_EDGES_DEV)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, lsm, ci, coast, stream
      integer(c_int), value :: nx, ny, halo, south, north, rule
    end function
    integer(c_int) function c_band_get_dist_dev(ctx, nx, ny, halo, south, north, coast, mask, lon, lat, maxdist, kwin, &
        cdist, stream) bind(C, name=SB_BAND_GET_DIST_DEV)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx, coast, mask, cdist, stream
      integer(c_int), value :: nx, ny, halo, south, north, kwin
      real(rk), value :: maxdist
      real(rk), intent(in) :: lon(*), lat(*)
    end function
    integer(c_int) function c_band_coast_open(ctx, nx, ny, halo, south, north, lon, lat, maxdist, kwin, rule, incremental) &
        bind(C, name=SB_BAND_COAST_OPEN)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, halo, south, north, kwin, rule, incremental
      real(rk), value :: maxdist
      real(rk), intent(in) :: lon(*), lat(*)
    end function
    integer(c_int) function c_band_ice_dev(ctx, lsm, ci, cdist, stream) bind(C, name=SB_BAND_ICE_DEV)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, lsm, ci, cdist, stream
    end function
    integer(c_int) function c_band_ice_report(ctx, rep) bind(C, name="sb_band_ice_report")
      import :: c_ptr, c_int, c_long_long
      type(c_ptr), value :: ctx
      integer(c_long_long), intent(inout) :: rep(4)
    end function
    integer(c_int) function c_band_coast_close(ctx) bind(C, name="sb_band_coast_close")
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function c_um_coast_open(ctx, nx, ny, hi, hj, wi, wj, tlat, tlon, maxdist, incremental) &
        bind(C, name=SB_UM_COAST_OPEN)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, hi, hj, wi, wj, incremental
      real(rk), value :: maxdist
      real(rk), intent(in) :: tlat(*), tlon(*)
    end function
    integer(c_int) function c_um_ice(ctx, lf, ci, cdist) bind(C, name=SB_UM_ICE)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      real(rk), intent(in) :: lf(*), ci(*)
      real(rk), intent(inout) :: cdist(*)
    end function
    integer(c_int) function c_um_ice_dev(ctx, lf, ci, cdist, stream) bind(C, name=SB_UM_ICE_DEV)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, lf, ci, cdist, stream
    end function
    integer(c_int) function c_um_ice_report(ctx, rep) bind(C, name="sb_um_ice_report")
      import :: c_ptr, c_int, c_long_long
      type(c_ptr), value :: ctx
      integer(c_long_long), intent(inout) :: rep(4)
    end function
    integer(c_int) function c_um_coast_close(ctx) bind(C, name="sb_um_coast_close")
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function c_um_tile_coast_open(ctx, nx, ny, hi, hj, wi, wj, beyond, tlat_l, tlon_l, maxdist, incremental) &
        bind(C, name=SB_UM_TILE_COAST_OPEN)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      integer(c_int), value :: nx, ny, hi, hj, wi, wj, incremental
      integer(c_int), intent(in) :: beyond(4)
      real(rk), value :: maxdist
      real(rk), intent(in) :: tlat_l(*), tlon_l(*)
    end function
    integer(c_int) function c_um_tile_ice(ctx, lf, ci, cdist) bind(C, name=SB_UM_TILE_ICE)
      import :: c_ptr, c_int, rk
      type(c_ptr), value :: ctx
      real(rk), intent(in) :: lf(*), ci(*)
      real(rk), intent(inout) :: cdist(*)
    end function
    integer(c_int) function c_um_tile_ice_dev(ctx, lf, ci, cdist, stream) bind(C, name=SB_UM_TILE_ICE_DEV)
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx, lf, ci, cdist, stream
    end function
    integer(c_int) function c_um_tile_ice_report(ctx, rep) bind(C, name="sb_um_tile_ice_report")
      import :: c_ptr, c_int, c_long_long
      type(c_ptr), value :: ctx
      integer(c_long_long), intent(inout) :: rep(4)
    end function
    integer(c_int) function c_um_tile_coast_close(ctx) bind(C, name="sb_um_tile_coast_close")
      import :: c_ptr, c_int
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function c_search_radius(ctx, nx, ny, halo, bnd, mask, maxdist, radius, summary, hist, nhist) &
        bind(C, name=SB_SEARCH_RADIUS)
      import :: c_ptr, c_int, c_long_long, rk
      type(c_ptr), value :: ctx, hist
      integer(c_int), value :: nx, ny, halo, bnd, nhist
      real(rk), value :: maxdist
      real(rk), intent(in) :: mask(*)
      integer(c_int), intent(inout) :: radius(*)
      integer(c_long_long), intent(inout) :: summary(4)
    end function
    integer(c_int) function c_band_search_radius(ctx, nx, ny, halo, south, north, mask, maxdist, radius, summary, hist, nhist) &
        bind(C, name=SB_BAND_SEARCH_RADIUS)
      import :: c_ptr, c_int, c_long_long, rk
      type(c_ptr), value :: ctx, hist
      integer(c_int), value :: nx, ny, halo, south, north, nhist
      real(rk), value :: maxdist
      real(rk), intent(in) :: mask(*)
      integer(c_int), intent(inout) :: radius(*)
      integer(c_long_long), intent(inout) :: summary(4)
    end function
  end interface

contains

  !> Release the device context (optional; a host model may call it at shutdown).
  subroutine sb_shutdown()
    call sb_release_ctx()
  end subroutine sb_shutdown

  !---------------------------------------------------------------------------
  ! ref: generic/sea_breeze_diag.f90:55-56 -- same dummy order
  !---------------------------------------------------------------------------
  subroutine seabreeze_diag(timestep, timestep_number, &
      p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con)
    integer, intent(in) :: timestep_number
    real, intent(in), contiguous :: p(:,:,:), u(:,:,:), v(:,:,:), theta(:,:)
    real, intent(in) :: timestep
    real, intent(in), contiguous :: mask(:,:), z(:,:), sigma(:,:)
    real, intent(inout), contiguous :: sb_con(:,:), windspeed(:,:), winddir(:,:), thc(:,:)
    integer :: error
    call seabreeze_diag_status(timestep, timestep_number, p, u, v, theta, mask, z, sigma, &
                               windspeed, winddir, thc, sb_con, error)
    if (error /= 0) call fail('seabreeze_diag', int(error, c_int))
  end subroutine seabreeze_diag

  !> Same call with the UM-style status out-argument instead of stopping
  !! (ref: UM/vn10.7/sea_breeze_diag.F90:55-56,102: error = 0 ok, 1 bad dimensions).
  subroutine seabreeze_diag_status(timestep, timestep_number, &
      p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con, error)
    integer, intent(in) :: timestep_number
    real, intent(in), contiguous :: p(:,:,:), u(:,:,:), v(:,:,:), theta(:,:)
    real, intent(in) :: timestep
    real, intent(in), contiguous :: mask(:,:), z(:,:), sigma(:,:)
    real, intent(inout), contiguous :: sb_con(:,:), windspeed(:,:), winddir(:,:), thc(:,:)
    integer, intent(out) :: error
    integer(c_int) :: nx, ny, nz, h, bnd
    nx = size(p, 1); ny = size(p, 2); nz = size(p, 3)       ! ref :145-153: the loop extent is p's
    error = 1
    if (nx < 1 .or. ny < 1 .or. nz < 1) return               ! ref: UM copy :198-202
    if (any(shape(u) /= shape(p)) .or. any(shape(v) /= shape(p))) return
    if (any(shape(windspeed) /= [nx, ny]) .or. any(shape(winddir) /= [nx, ny]) .or. &
        any(shape(thc) /= [nx, ny]) .or. any(shape(sb_con) /= [nx, ny])) return
    if (any(shape(mask) /= shape(theta)) .or. any(shape(z) /= shape(theta)) .or. &
        any(shape(sigma) /= shape(theta))) return
    if (size(theta, 1) == nx .and. size(theta, 2) == ny) then
      h = 0; bnd = SB_BND_GLOBAL
    else
      h = (size(theta, 1) - nx) / 2; bnd = SB_BND_HALO
      if (h < 1 .or. size(theta, 1) /= nx + 2*h .or. size(theta, 2) /= ny + 2*h) return
    end if
    call ensure_ctx()
    error = c_seabreeze_diag(ctx, real(timestep, rk), int(timestep_number, c_int), nx, ny, nz, h, bnd, &
                             p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con, c_null_ptr)
  end subroutine seabreeze_diag_status

  !---------------------------------------------------------------------------
  ! The Unified Model hook's argument list and field bounds
  ! (ref: UM/vn10.7/sea_breeze_diag.F90:55-56,66-117): (theta, z, sigma, mask) in the UM's order, `error` last;
  ! p, u, v and the four state fields on pdims/tdims (nx, ny[, nz]); theta, z, sigma on tdims_s (small halo) and
  ! mask on tdims_l (large halo) -- the halo widths are read off the array shapes.  theta is intent(inout) as in
  ! the UM copy: with SB_UM_THETA_TO_T0 in `flags` it comes back as t0 (:210-211); SB_UM_LEVEL_WALK selects the UM
  ! copy's level rule (:265-274).  flags absent: both, i.e. the UM copy's behaviour.
  !---------------------------------------------------------------------------
  subroutine seabreeze_diag_um(timestep, timestep_number, &
      p, u, v, theta, z, sigma, mask, windspeed, winddir, thc, sb_con, error, flags)
    integer, intent(in) :: timestep_number
    real, intent(in) :: timestep
    real, intent(in), contiguous :: p(:,:,:), u(:,:,:), v(:,:,:), z(:,:), sigma(:,:), mask(:,:)
    real, intent(inout), contiguous :: theta(:,:), sb_con(:,:), windspeed(:,:), winddir(:,:), thc(:,:)
    integer, intent(out) :: error
    integer, intent(in), optional :: flags
    integer(c_int) :: nx, ny, nz, hs, hl, fl, err, rc
    nx = size(p, 1); ny = size(p, 2); nz = size(p, 3)
    error = 1
    if (nx < 1 .or. ny < 1 .or. nz < 1) return               ! ref: UM copy :198-202
    if (any(shape(u) /= shape(p)) .or. any(shape(v) /= shape(p))) return
    if (any(shape(windspeed) /= [nx, ny]) .or. any(shape(winddir) /= [nx, ny]) .or. &
        any(shape(thc) /= [nx, ny]) .or. any(shape(sb_con) /= [nx, ny])) return
    hs = (size(theta, 1) - nx) / 2
    hl = (size(mask, 1) - nx) / 2
    if (hs < 0 .or. hl < hs) return
    if (any(shape(theta) /= [nx + 2*hs, ny + 2*hs]) .or. any(shape(z) /= shape(theta)) .or. &
        any(shape(sigma) /= shape(theta)) .or. any(shape(mask) /= [nx + 2*hl, ny + 2*hl])) return
    fl = SB_UM_THETA_TO_T0 + SB_UM_LEVEL_WALK
    if (present(flags)) fl = int(flags, c_int)
    call ensure_ctx()
    rc = c_diag_um(ctx, real(timestep, rk), int(timestep_number, c_int), nx, ny, nz, hs, hl, p, u, v, theta, z, sigma, &
                   mask, windspeed, winddir, thc, sb_con, fl, err)
    if (rc /= 0) call fail('seabreeze_diag_um', rc)
    error = int(err)
  end subroutine seabreeze_diag_um

  !---------------------------------------------------------------------------
  ! One step of a latitude band of a multi-GPU run (one process per GPU, sb_comm_init done).
  ! Arguments as seabreeze_diag for this band's rows; theta, mask, z, sigma carry h ghost cells
  ! all round ((nx+2h, ny+2h), h >= 1).  mask, z, sigma are static: fill their ghost cells once
  ! with halo_exchange_mod::swap_bounds.  theta's ghost cells are filled inside the call (and
  ! returned), overlapped with the kernels that do not need them; the sigma statistics are
  ! reduced over all bands, so every band reproduces the rows of the single-domain result.
  ! ref: generic/sea_breeze_diag.f90:55-271 + the exchange its UM twin makes,
  !      UM/vn10.7/sea_breeze_diag.F90:408-410
  !---------------------------------------------------------------------------
  subroutine band_seabreeze_diag(timestep, timestep_number, &
      p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con)
    integer, intent(in) :: timestep_number
    real, intent(in), contiguous :: p(:,:,:), u(:,:,:), v(:,:,:)
    real, intent(in) :: timestep
    real, intent(inout), contiguous :: theta(:,:)
    real, intent(in), contiguous :: mask(:,:), z(:,:), sigma(:,:)
    real, intent(inout), contiguous :: sb_con(:,:), windspeed(:,:), winddir(:,:), thc(:,:)
    integer(c_int) :: nx, ny, nz, h, rc
    nx = size(p, 1); ny = size(p, 2); nz = size(p, 3)
    h = (size(theta, 1) - nx) / 2
    if (h < 1 .or. size(theta, 1) /= nx + 2*h .or. size(theta, 2) /= ny + 2*h .or. &
        any(shape(mask) /= shape(theta)) .or. any(shape(z) /= shape(theta)) .or. any(shape(sigma) /= shape(theta)) .or. &
        any(shape(u) /= shape(p)) .or. any(shape(v) /= shape(p)) .or. &
        any(shape(windspeed) /= [nx, ny]) .or. any(shape(winddir) /= [nx, ny]) .or. &
        any(shape(thc) /= [nx, ny]) .or. any(shape(sb_con) /= [nx, ny])) &
      call fail('band_seabreeze_diag: theta, mask, z, sigma must be (nx+2h, ny+2h) with h >= 1', 1_c_int)
    call ensure_ctx()
    rc = c_band_diag(ctx, real(timestep, rk), int(timestep_number, c_int), nx, ny, nz, h, &
                     p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con, c_null_ptr)
    if (rc /= 0) call fail('band_seabreeze_diag', rc)
  end subroutine band_seabreeze_diag

  !---------------------------------------------------------------------------
  ! Device-resident forms: every array argument is a device pointer (sb_context_mod::sb_dev_alloc),
  ! Fortran order as above; the call only enqueues on the context's stream
  ! (sb_context_mod::sb_device_synchronize waits).  halo = 0: single global domain.
  !---------------------------------------------------------------------------
  subroutine seabreeze_diag_dev(timestep, timestep_number, nx, ny, nz, halo, &
      p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con)
    integer, intent(in) :: timestep_number, nx, ny, nz, halo
    real, intent(in) :: timestep
    type(c_ptr), intent(in) :: p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con
    integer(c_int) :: rc, bnd
    bnd = SB_BND_GLOBAL
    if (halo > 0) bnd = SB_BND_HALO
    call ensure_ctx()
    rc = c_diag_dev(ctx, real(timestep, rk), int(timestep_number, c_int), int(nx, c_int), int(ny, c_int), &
                    int(nz, c_int), int(halo, c_int), bnd, p, u, v, theta, mask, z, sigma, &
                    windspeed, winddir, thc, sb_con, c_null_ptr, c_null_ptr)
    if (rc /= 0) call fail('seabreeze_diag_dev', rc)
  end subroutine seabreeze_diag_dev

  subroutine band_seabreeze_diag_dev(timestep, timestep_number, nx, ny, nz, halo, &
      p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con)
    integer, intent(in) :: timestep_number, nx, ny, nz, halo
    real, intent(in) :: timestep
    type(c_ptr), intent(in) :: p, u, v, theta, mask, z, sigma, windspeed, winddir, thc, sb_con
    integer(c_int) :: rc
    call ensure_ctx()
    rc = c_band_diag_dev(ctx, real(timestep, rk), int(timestep_number, c_int), int(nx, c_int), int(ny, c_int), &
                         int(nz, c_int), int(halo, c_int), p, u, v, theta, mask, z, sigma, &
                         windspeed, winddir, thc, sb_con, c_null_ptr, c_null_ptr)
    if (rc /= 0) call fail('band_seabreeze_diag_dev', rc)
  end subroutine band_seabreeze_diag_dev

  !---------------------------------------------------------------------------
  ! ref: generic/sea_breeze_diag.f90:273-373.  landfrac/icefrac are (nx, ny); the coast
  ! mask is written into mask(1+halo_size : nx+halo_size, 1+halo_size : ny+halo_size)
  ! exactly as :369 does, then the ghost cells are filled by swap_bounds (:371).
  !---------------------------------------------------------------------------
  subroutine get_edges(mask, icefrac, landfrac, halo_size)
    use halo_exchange_mod, only : swap_bounds
    integer, intent(in) :: halo_size
    real, intent(out) :: mask(:,:)
    real, intent(in), contiguous :: landfrac(:,:), icefrac(:,:)
    real, allocatable :: coast(:,:)
    integer(c_int) :: nx, ny, rc
    nx = size(landfrac, 1); ny = size(landfrac, 2)
    if (size(mask, 1) < nx + halo_size .or. size(mask, 2) < ny + halo_size) &
      call fail('get_edges: mask smaller than landfrac + halo_size', 1_c_int)
    allocate(coast(nx, ny))
    call ensure_ctx()
    rc = c_get_edges(ctx, nx, ny, landfrac, icefrac, 1_c_int, SB_BND_GLOBAL, coast)
    if (rc /= 0) call fail('get_edges', rc)
    mask = 0.
    mask(1+halo_size:nx+halo_size, 1+halo_size:ny+halo_size) = coast
    deallocate(coast)
    call swap_bounds(mask, halo_size)
  end subroutine get_edges

  !---------------------------------------------------------------------------
  ! ref: generic/sea_breeze_diag.f90:375-455.  coast is either (nlons, nlats) or the
  ! ghost-celled mask get_edges wrote (interior at offset halo_size, as the reference's
  ! caller passes it, ref: generic/dummy_model.f90:32-34); the window is +-halo_size cells
  ! (:422,:425) and the sign comes from landfrac > 0 (:442).
  !---------------------------------------------------------------------------
  subroutine get_dist_r(coast, landfrac, lon, lat, maxdist, cdist, halo_size)
    integer, intent(in) :: halo_size
    real, intent(in), contiguous :: lon(:), lat(:), landfrac(:,:)
    real, intent(in) :: coast(:,:)
    real, intent(in) :: maxdist
    real, intent(out), contiguous :: cdist(:,:)
    real, allocatable :: c2(:,:)
    integer(c_int) :: nx, ny, rc
    nx = size(lon, 1); ny = size(lat, 1)
    if (any(shape(landfrac) /= [nx, ny]) .or. any(shape(cdist) /= [nx, ny])) &
      call fail('get_dist: landfrac/cdist must be (size(lon), size(lat))', 1_c_int)
    allocate(c2(nx, ny))
    if (size(coast, 1) == nx .and. size(coast, 2) == ny) then
      c2 = coast
    else if (size(coast, 1) >= nx + halo_size .and. size(coast, 2) >= ny + halo_size) then
      c2 = coast(1+halo_size:nx+halo_size, 1+halo_size:ny+halo_size)
    else
      call fail('get_dist: coast has neither the grid shape nor the ghost-celled shape', 1_c_int)
    end if
    call ensure_ctx()
    rc = c_get_dist(ctx, nx, ny, c2, landfrac, lon, lat, real(maxdist, rk), int(halo_size, c_int), cdist)
    if (rc /= 0) call fail('get_dist', rc)
    deallocate(c2)
  end subroutine get_dist_r

  subroutine get_dist_i(coast, landfrac, lon, lat, maxdist, cdist, halo_size)
    integer, intent(in) :: halo_size, maxdist
    real, intent(in), contiguous :: lon(:), lat(:), landfrac(:,:)
    real, intent(in) :: coast(:,:)
    real, intent(out), contiguous :: cdist(:,:)
    call get_dist_r(coast, landfrac, lon, lat, real(maxdist), cdist, halo_size)
  end subroutine get_dist_i

  !---------------------------------------------------------------------------
  ! get_edges and get_dist for ONE LATITUDE BAND of a multi-GPU run: the dummy order of the generic routines plus the
  ! band arguments.  Every field is in the band step's frame, (nx+2*halo_size, ny+2*halo_size) with the band's own
  ! rows in the interior; lon has nx entries, lat ny+2*halo_size (one per frame row).  south / north: the band touches
  ! that pole.  On a cut side the ghost rows next to the interior are read -- one row of landfrac and icefrac, kwin
  ! rows of coast -- and must have been filled (halo_exchange_mod::swap_bounds); ghost rows beyond a pole and the
  ! east-west ghost columns are never read.  Only the interior of mask / cdist is written: call swap_bounds on them
  ! afterwards.  The interior is the whole-grid routines' field, bit for bit.  The window is +-halo_size cells as in
  ! get_dist, or +-kwin <= halo_size where kwin is given.
  !---------------------------------------------------------------------------
  subroutine band_get_edges(mask, icefrac, landfrac, halo_size, south, north)
    integer, intent(in) :: halo_size
    logical, intent(in) :: south, north
    real, intent(inout), contiguous :: mask(:,:)
    real, intent(in), contiguous :: landfrac(:,:), icefrac(:,:)
    integer(c_int) :: nx, ny, rc
    nx = size(landfrac, 1) - 2*halo_size; ny = size(landfrac, 2) - 2*halo_size
    if (halo_size < 0 .or. nx < 1 .or. ny < 1 .or. any(shape(icefrac) /= shape(landfrac)) .or. &
        any(shape(mask) /= shape(landfrac))) &
      call fail('band_get_edges: mask, icefrac, landfrac must be (nx+2*halo_size, ny+2*halo_size)', 1_c_int)
    call ensure_ctx()
    rc = c_band_get_edges(ctx, nx, ny, int(halo_size, c_int), merge(1_c_int, 0_c_int, south), merge(1_c_int, 0_c_int, north), &
                          landfrac, icefrac, 1_c_int, mask)
    if (rc /= 0) call fail('band_get_edges', rc)
  end subroutine band_get_edges

  subroutine band_get_dist_r(coast, landfrac, lon, lat, maxdist, cdist, halo_size, south, north, kwin)
    integer, intent(in) :: halo_size
    logical, intent(in) :: south, north
    integer, intent(in), optional :: kwin
    real, intent(in), contiguous :: lon(:), lat(:), landfrac(:,:), coast(:,:)
    real, intent(in) :: maxdist
    real, intent(inout), contiguous :: cdist(:,:)
    integer(c_int) :: nx, ny, rc, k
    nx = size(lon, 1); ny = size(lat, 1) - 2*halo_size
    if (halo_size < 0 .or. ny < 1 .or. any(shape(coast) /= [nx + 2*halo_size, ny + 2*halo_size]) .or. &
        any(shape(landfrac) /= shape(coast)) .or. any(shape(cdist) /= shape(coast))) &
      call fail('band_get_dist: coast, landfrac, cdist must be (size(lon)+2*halo_size, size(lat)), lat one per frame row', &
                1_c_int)
    k = int(halo_size, c_int)
    if (present(kwin)) k = int(kwin, c_int)
    call ensure_ctx()
    rc = c_band_get_dist(ctx, nx, ny, int(halo_size, c_int), merge(1_c_int, 0_c_int, south), merge(1_c_int, 0_c_int, north), &
                         coast, landfrac, lon, lat, real(maxdist, rk), k, cdist)
    if (rc /= 0) call fail('band_get_dist', rc)
  end subroutine band_get_dist_r

  subroutine band_get_dist_i(coast, landfrac, lon, lat, maxdist, cdist, halo_size, south, north, kwin)
    integer, intent(in) :: halo_size, maxdist
    logical, intent(in) :: south, north
    integer, intent(in), optional :: kwin
    real, intent(in), contiguous :: lon(:), lat(:), landfrac(:,:), coast(:,:)
    real, intent(inout), contiguous :: cdist(:,:)
    call band_get_dist_r(coast, landfrac, lon, lat, real(maxdist), cdist, halo_size, south, north, kwin)
  end subroutine band_get_dist_i

  !---------------------------------------------------------------------------
  ! search_radius: the radius of every band cell's expanding window (ref: generic/sea_breeze_diag.f90:188-214) from the
  ! signed coast distance alone, before any seabreeze_diag call -- call it after get_dist, and again when the ice mask
  ! changes.  mask is (nx+2*halo_size, ny+2*halo_size): halo_size = 0 is the whole globe (longitude periodic, latitude
  ! clamped), halo_size > 0 a ghost-celled frame whose windows end at the frame.  radius (nx, ny): 0 off the band, the
  ! radius, or -1 where no window up to seabreeze_diag's own limit holds both classes (it returns NaN there).  summary:
  ! band cells, those with a radius, those with -1, the largest radius.  band_search_radius: one latitude band in the
  ! band step's frame (south / north: the band touches that pole); the ghost rows of mask on a cut side are read as
  ! swap_bounds left them, and with halo_size >= the whole grid's summary(4) the interior equals the whole grid's rows.
  !---------------------------------------------------------------------------
  subroutine search_radius(mask, maxdist, radius, summary, halo_size)
    real, intent(in), contiguous :: mask(:,:)
    real, intent(in) :: maxdist
    integer(c_int), intent(inout), contiguous :: radius(:,:)
    integer(c_long_long), intent(out) :: summary(4)
    integer, intent(in) :: halo_size
    integer(c_int) :: nx, ny, rc, bnd
    nx = size(mask, 1) - 2*halo_size; ny = size(mask, 2) - 2*halo_size
    if (halo_size < 0 .or. nx < 1 .or. ny < 1 .or. any(shape(radius) /= [nx, ny])) &
      call fail('search_radius: mask must be (nx+2*halo_size, ny+2*halo_size), radius (nx, ny)', 1_c_int)
    bnd = SB_BND_GLOBAL
    if (halo_size > 0) bnd = SB_BND_HALO
    call ensure_ctx()
    rc = c_search_radius(ctx, nx, ny, int(halo_size, c_int), bnd, mask, real(maxdist, rk), radius, summary, c_null_ptr, 0_c_int)
    if (rc /= 0) call fail('search_radius', rc)
  end subroutine search_radius

  subroutine band_search_radius(mask, maxdist, radius, summary, halo_size, south, north)
    real, intent(in), contiguous :: mask(:,:)
    real, intent(in) :: maxdist
    integer(c_int), intent(inout), contiguous :: radius(:,:)
    integer(c_long_long), intent(out) :: summary(4)
    integer, intent(in) :: halo_size
    logical, intent(in) :: south, north
    integer(c_int) :: nx, ny, rc
    nx = size(mask, 1) - 2*halo_size; ny = size(mask, 2) - 2*halo_size
    if (halo_size < 0 .or. nx < 1 .or. ny < 1 .or. any(shape(radius) /= [nx, ny])) &
      call fail('band_search_radius: mask must be (nx+2*halo_size, ny+2*halo_size), radius (nx, ny)', 1_c_int)
    call ensure_ctx()
    rc = c_band_search_radius(ctx, nx, ny, int(halo_size, c_int), merge(1_c_int, 0_c_int, south), &
                              merge(1_c_int, 0_c_int, north), mask, real(maxdist, rk), radius, summary, c_null_ptr, 0_c_int)
    if (rc /= 0) call fail('band_search_radius', rc)
  end subroutine band_search_radius

  ! Device-resident forms: the fields are device pointers (sb_context_mod::sb_dev_alloc) in the same frames, lon and lat
  ! host arrays; the calls only enqueue on the context's stream.
  subroutine band_get_edges_dev(mask, icefrac, landfrac, nx, ny, halo_size, south, north)
    type(c_ptr), intent(in) :: mask, icefrac, landfrac
    integer, intent(in) :: nx, ny, halo_size
    logical, intent(in) :: south, north
    integer(c_int) :: rc
    call ensure_ctx()
    rc = c_band_get_edges_dev(ctx, int(nx, c_int), int(ny, c_int), int(halo_size, c_int), merge(1_c_int, 0_c_int, south), &
                              merge(1_c_int, 0_c_int, north), landfrac, icefrac, 1_c_int, mask, c_null_ptr)
    if (rc /= 0) call fail('band_get_edges_dev', rc)
  end subroutine band_get_edges_dev

  subroutine band_get_dist_dev(coast, landfrac, lon, lat, maxdist, cdist, halo_size, south, north, kwin)
    type(c_ptr), intent(in) :: coast, landfrac, cdist
    real, intent(in), contiguous :: lon(:), lat(:)
    real, intent(in) :: maxdist
    integer, intent(in) :: halo_size
    logical, intent(in) :: south, north
    integer, intent(in), optional :: kwin
    integer(c_int) :: rc, k
    k = int(halo_size, c_int)
    if (present(kwin)) k = int(kwin, c_int)
    call ensure_ctx()
    rc = c_band_get_dist_dev(ctx, int(size(lon), c_int), int(size(lat) - 2*halo_size, c_int), int(halo_size, c_int), &
                             merge(1_c_int, 0_c_int, south), merge(1_c_int, 0_c_int, north), coast, landfrac, lon, lat, &
                             real(maxdist, rk), k, cdist, c_null_ptr)
    if (rc /= 0) call fail('band_get_dist_dev', rc)
  end subroutine band_get_dist_dev

  ! A band whose coast moves with the sea ice (include/seabreeze_hip.h: sb_band_coast_open): open once per land mask --
  ! lon (nx) and lat (ny + 2*halo_size, one per frame row) are host arrays and are copied; a cut side needs
  ! kwin + 1 <= halo_size -- then band_ice_dev per ice plane: landfrac, icefrac and cdist are device frames in the band
  ! step's layout, and the call only enqueues on the context's stream.  What the caller exchanges per plane: the ghost rows
  ! of icefrac before the call, the ghost cells of cdist after it; no coast travels.
  subroutine band_coast_open(lon, lat, maxdist, halo_size, south, north, kwin, rule, incremental)
    real, intent(in), contiguous :: lon(:), lat(:)
    real, intent(in) :: maxdist
    integer, intent(in) :: halo_size, kwin
    logical, intent(in) :: south, north
    integer, intent(in), optional :: rule
    logical, intent(in), optional :: incremental
    integer(c_int) :: rc, r, inc
    r = 1_c_int
    if (present(rule)) r = int(rule, c_int)
    inc = 1_c_int
    if (present(incremental)) inc = merge(1_c_int, 0_c_int, incremental)
    call ensure_ctx()
    rc = c_band_coast_open(ctx, int(size(lon), c_int), int(size(lat) - 2*halo_size, c_int), int(halo_size, c_int), &
                           merge(1_c_int, 0_c_int, south), merge(1_c_int, 0_c_int, north), lon, lat, real(maxdist, rk), &
                           int(kwin, c_int), r, inc)
    if (rc /= 0) call fail('band_coast_open', rc)
  end subroutine band_coast_open

  subroutine band_ice_dev(landfrac, icefrac, cdist)
    type(c_ptr), intent(in) :: landfrac, icefrac, cdist
    integer(c_int) :: rc
    call ensure_ctx()
    rc = c_band_ice_dev(ctx, landfrac, icefrac, cdist, c_null_ptr)
    if (rc /= 0) call fail('band_ice_dev', rc)
  end subroutine band_ice_dev

  ! (synchronises) calls since the open / those after the first whose coast differed (-1: every call computes the whole
  ! band) / (own row, tile) pairs the last call marked / pairs of the band
  subroutine band_ice_report(rep)
    integer(c_long_long), intent(out) :: rep(4)
    integer(c_int) :: rc
    call ensure_ctx()
    rep = 0
    rc = c_band_ice_report(ctx, rep)
    if (rc /= 0) call fail('band_ice_report', rc)
  end subroutine band_ice_report

  subroutine band_coast_close()
    integer(c_int) :: rc
    call ensure_ctx()
    rc = c_band_coast_close(ctx)
    if (rc /= 0) call fail('band_coast_close', rc)
  end subroutine band_coast_close

  !---------------------------------------------------------------------------
  ! The UM copy's get_edges(mask, icefrac, landfrac) (ref: UM/vn10.7/sea_breeze_diag.F90:328-446) in its argument
  ! order and bounds: landfrac, icefrac on tdims (nx, ny), mask on tdims_l (nx+2*halo_i, ny+2*halo_j) -- the halo
  ! widths are read off the shapes.  The land rule is applied to the interior and to the one-cell ring round it; the
  ! ring's landfrac/icefrac are the domain's edge cells (what a single-domain run's swap_bounds of the mask gives at
  ! a limited-area edge).  Only the interior of mask is written: its ghost cells are left to the caller's
  ! swap_bounds (the UM's closing call, :440-442).
  !---------------------------------------------------------------------------
  subroutine get_edges_um(mask, icefrac, landfrac)
    real, intent(inout), contiguous :: mask(:,:)
    real, intent(in), contiguous :: icefrac(:,:), landfrac(:,:)
    real, allocatable :: lf(:,:), ci(:,:)
    integer(c_int) :: nx, ny, hi, hj, rc
    integer :: i, j
    nx = size(landfrac, 1); ny = size(landfrac, 2)
    hi = (size(mask, 1) - nx) / 2; hj = (size(mask, 2) - ny) / 2
    if (any(shape(icefrac) /= [nx, ny]) .or. hi < 1 .or. hj < 1 .or. &
        any(shape(mask) /= [nx + 2*hi, ny + 2*hj])) &
      call fail('get_edges_um: need landfrac, icefrac (nx, ny) and mask (nx+2*halo_i, ny+2*halo_j), halos >= 1', 1_c_int)
    allocate(lf(nx + 2*hi, ny + 2*hj), ci(nx + 2*hi, ny + 2*hj))
    do j = 1, ny + 2*hj
      do i = 1, nx + 2*hi
        lf(i, j) = landfrac(min(max(i - hi, 1), nx), min(max(j - hj, 1), ny))
        ci(i, j) = icefrac(min(max(i - hi, 1), nx), min(max(j - hj, 1), ny))
      end do
    end do
    call ensure_ctx()
    rc = c_get_edges_um(ctx, nx, ny, hi, hj, lf, ci, mask)
    if (rc /= 0) call fail('get_edges_um', rc)
    deallocate(lf, ci)
  end subroutine get_edges_um

  !---------------------------------------------------------------------------
  ! The UM copy's get_dist(landfrac, coast) (ref: UM/vn10.7/sea_breeze_diag.F90:448-601) in its argument order:
  ! coast on tdims_l (nx+2*halo_i, ny+2*halo_j) is overwritten with the signed coast distance, as the UM does
  ! (:590-594); landfrac and the 2-D coordinates true_latitude, true_longitude (degrees, trignometric_mod's fields,
  ! :523-524) on tdims (nx, ny).  The window is +-halo_i columns x +-halo_j rows (:515-516), read off the shapes.
  ! maxdist: the UM's parameter of 180 km when absent.  Only the interior of coast is written: its ghost cells are
  ! left to the caller's swap_bounds (:598-600).
  !---------------------------------------------------------------------------
  subroutine get_dist_um(landfrac, coast, true_latitude, true_longitude, maxdist)
    real, intent(in), contiguous :: landfrac(:,:), true_latitude(:,:), true_longitude(:,:)
    real, intent(inout), contiguous :: coast(:,:)
    real, intent(in), optional :: maxdist
    real, allocatable :: c2(:,:)
    real :: md
    integer(c_int) :: nx, ny, hi, hj, rc
    nx = size(landfrac, 1); ny = size(landfrac, 2)
    hi = (size(coast, 1) - nx) / 2; hj = (size(coast, 2) - ny) / 2
    if (any(shape(true_latitude) /= [nx, ny]) .or. any(shape(true_longitude) /= [nx, ny]) .or. hi < 0 .or. hj < 0 &
        .or. any(shape(coast) /= [nx + 2*hi, ny + 2*hj])) &
      call fail('get_dist_um: need landfrac, true_latitude, true_longitude (nx, ny), coast (nx+2*halo_i, ny+2*halo_j)', &
                1_c_int)
    md = 180.
    if (present(maxdist)) md = maxdist
    allocate(c2(size(coast, 1), size(coast, 2)))
    c2 = coast                                   ! (the coast mask the distance field replaces)
    call ensure_ctx()
    rc = c_get_dist_um(ctx, nx, ny, hi, hj, c2, landfrac, true_latitude, true_longitude, real(md, rk), coast)
    if (rc /= 0) call fail('get_dist_um', rc)
    deallocate(c2)
  end subroutine get_dist_um

  !---------------------------------------------------------------------------
  ! get_dist_um with the window stated apart from the layout: +-win_i columns x +-win_j rows, each 0 .. 255
  ! (SB_DIST_UM_MAX_WINDOW; 113 cells at 0.0135 degrees and 180 km), wider or narrower than the ghost width of coast,
  ! which is read off the shapes and only says where the interior lies.  Everything else is get_dist_um's.
  !---------------------------------------------------------------------------
  subroutine get_dist_um_win(landfrac, coast, true_latitude, true_longitude, win_i, win_j, maxdist)
    real, intent(in), contiguous :: landfrac(:,:), true_latitude(:,:), true_longitude(:,:)
    real, intent(inout), contiguous :: coast(:,:)
    integer, intent(in) :: win_i, win_j
    real, intent(in), optional :: maxdist
    real, allocatable :: c2(:,:)
    real :: md
    integer(c_int) :: nx, ny, hi, hj, rc
    nx = size(landfrac, 1); ny = size(landfrac, 2)
    hi = (size(coast, 1) - nx) / 2; hj = (size(coast, 2) - ny) / 2
    if (any(shape(true_latitude) /= [nx, ny]) .or. any(shape(true_longitude) /= [nx, ny]) .or. hi < 0 .or. hj < 0 &
        .or. any(shape(coast) /= [nx + 2*hi, ny + 2*hj])) &
      call fail('get_dist_um_win: need landfrac, true_latitude, true_longitude (nx, ny), coast (nx+2*halo_i, ny+2*halo_j)', &
                1_c_int)
    md = 180.
    if (present(maxdist)) md = maxdist
    allocate(c2(size(coast, 1), size(coast, 2)))
    c2 = coast                                   ! (the coast mask the distance field replaces)
    call ensure_ctx()
    rc = c_get_dist_um_win(ctx, nx, ny, hi, hj, int(win_i, c_int), int(win_j, c_int), c2, landfrac, true_latitude, &
                           true_longitude, real(md, rk), coast)
    if (rc /= 0) call fail('get_dist_um_win', rc)
    deallocate(c2)
  end subroutine get_dist_um_win

  !---------------------------------------------------------------------------
  ! The UM-layout coast setup on one tile of a 2-D domain decomposition (include/seabreeze_hip.h: sb_tile_get_edges_um,
  ! sb_tile_get_dist_um): every field is the rank's frame on tdims_l, (nx+2*halo_i, ny+2*halo_j), its ghost cells filled by
  ! the caller's swap_bounds -- the coordinate frames included; all frames have one shape, so the halo widths are stated.
  ! sides: a sum of SB_TILE_* (a set bit: that side is the domain's edge; a clear one: a cut).  tile_get_edges_um writes 0/1
  ! into the interior of coast_l and ext_i ghost columns / ext_j ghost rows beyond it on every cut side (halo >= ext + 1
  ! there), so a rank forms the coast of the ghost cells its window reads; tile_get_dist_um overwrites the interior of
  ! coast_l with the signed distance, as get_dist_um does, its sources being the coast cells of the interior and of the
  ! ghost cells within the window on every cut side (halo >= win there).  The interior equals the tile's cells of the
  ! whole-domain get_edges_um + get_dist_um_win.
  !---------------------------------------------------------------------------
  subroutine tile_get_edges_um(landfrac_l, icefrac_l, coast_l, halo_i, halo_j, ext_i, ext_j, sides)
    real, intent(in), contiguous :: landfrac_l(:,:), icefrac_l(:,:)
    real, intent(inout), contiguous :: coast_l(:,:)
    integer, intent(in) :: halo_i, halo_j, ext_i, ext_j, sides
    integer(c_int) :: nx, ny, rc
    nx = size(coast_l, 1) - 2*halo_i; ny = size(coast_l, 2) - 2*halo_j
    if (any(shape(landfrac_l) /= shape(coast_l)) .or. any(shape(icefrac_l) /= shape(coast_l)) .or. nx < 1 .or. ny < 1) &
      call fail('tile_get_edges_um: need landfrac_l, icefrac_l, coast_l (nx+2*halo_i, ny+2*halo_j)', 1_c_int)
    call ensure_ctx()
    rc = c_tile_get_edges_um(ctx, nx, ny, int(halo_i, c_int), int(halo_j, c_int), int(ext_i, c_int), int(ext_j, c_int), &
                             int(sides, c_int), landfrac_l, icefrac_l, coast_l)
    if (rc /= 0) call fail('tile_get_edges_um', rc)
  end subroutine tile_get_edges_um

  subroutine tile_get_dist_um(landfrac_l, coast_l, true_latitude_l, true_longitude_l, halo_i, halo_j, win_i, win_j, sides, &
                              maxdist)
    real, intent(in), contiguous :: landfrac_l(:,:), true_latitude_l(:,:), true_longitude_l(:,:)
    real, intent(inout), contiguous :: coast_l(:,:)
    integer, intent(in) :: halo_i, halo_j, win_i, win_j, sides
    real, intent(in), optional :: maxdist
    real, allocatable :: c2(:,:)
    real :: md
    integer(c_int) :: nx, ny, rc
    nx = size(coast_l, 1) - 2*halo_i; ny = size(coast_l, 2) - 2*halo_j
    if (any(shape(landfrac_l) /= shape(coast_l)) .or. any(shape(true_latitude_l) /= shape(coast_l)) .or. &
        any(shape(true_longitude_l) /= shape(coast_l)) .or. nx < 1 .or. ny < 1) &
      call fail('tile_get_dist_um: need landfrac_l, coast_l, true_latitude_l, true_longitude_l (nx+2*halo_i, ny+2*halo_j)', &
                1_c_int)
    md = 180.
    if (present(maxdist)) md = maxdist
    allocate(c2(size(coast_l, 1), size(coast_l, 2)))
    c2 = coast_l                                 ! (the coast mask the distance field replaces)
    call ensure_ctx()
    rc = c_tile_get_dist_um(ctx, nx, ny, int(halo_i, c_int), int(halo_j, c_int), int(win_i, c_int), int(win_j, c_int), &
                            int(sides, c_int), c2, landfrac_l, true_latitude_l, true_longitude_l, real(md, rk), coast_l)
    if (rc /= 0) call fail('tile_get_dist_um', rc)
    deallocate(c2)
  end subroutine tile_get_dist_um

  !---------------------------------------------------------------------------
  ! A UM-layout coast that moves with the sea ice (include/seabreeze_hip.h: sb_um_coast_open): the UM rebuilds its mask
  ! from icefrac inside the timestep routine (ref: UM/vn10.7/sea_breeze_diag.F90:384-445); get_edges_um + get_dist_um_win
  ! per step would compute the whole interior again.  Open once per landfrac -- true_latitude, true_longitude on tdims
  ! (nx, ny), degrees, are copied; halo_i, halo_j >= 1 are the ghost widths of the tdims_l arrays of the ice calls, the
  ! window is +-win_i x +-win_j, each 0 .. 255 -- then um_ice per ice frame: landfrac_l, icefrac_l and cdist_l on tdims_l
  ! (nx+2*halo_i, ny+2*halo_j), the one-cell ring of the first two filled.  Only the interior of cdist_l is written, and
  ! what a call left there must still be there at the next one (later calls compute only what the moved coast can
  ! reach).  um_ice_dev takes device frames and only enqueues on the context's stream.
  !---------------------------------------------------------------------------
  subroutine um_coast_open(true_latitude, true_longitude, halo_i, halo_j, win_i, win_j, maxdist, incremental)
    real, intent(in), contiguous :: true_latitude(:,:), true_longitude(:,:)
    integer, intent(in) :: halo_i, halo_j, win_i, win_j
    real, intent(in), optional :: maxdist
    logical, intent(in), optional :: incremental
    real :: md
    integer(c_int) :: rc, inc
    if (any(shape(true_longitude) /= shape(true_latitude))) &
      call fail('um_coast_open: need true_latitude, true_longitude (nx, ny)', 1_c_int)
    md = 180.
    if (present(maxdist)) md = maxdist
    inc = 1_c_int
    if (present(incremental)) inc = merge(1_c_int, 0_c_int, incremental)
    call ensure_ctx()
    rc = c_um_coast_open(ctx, int(size(true_latitude, 1), c_int), int(size(true_latitude, 2), c_int), int(halo_i, c_int), &
                         int(halo_j, c_int), int(win_i, c_int), int(win_j, c_int), true_latitude, true_longitude, &
                         real(md, rk), inc)
    if (rc /= 0) call fail('um_coast_open', rc)
    um_shape = [int(size(true_latitude, 1), c_int), int(size(true_latitude, 2), c_int), int(halo_i, c_int), int(halo_j, c_int)]
  end subroutine um_coast_open

  subroutine um_ice(landfrac_l, icefrac_l, cdist_l)
    real, intent(in), contiguous :: landfrac_l(:,:), icefrac_l(:,:)
    real, intent(inout), contiguous :: cdist_l(:,:)
    integer(c_int) :: rc
    integer :: want(2)
    want = [um_shape(1) + 2*um_shape(3), um_shape(2) + 2*um_shape(4)]
    if (um_shape(1) < 1) call fail('um_ice without um_coast_open', 1_c_int)
    if (any(shape(landfrac_l) /= want) .or. any(shape(icefrac_l) /= want) .or. any(shape(cdist_l) /= want)) &
      call fail('um_ice: need landfrac_l, icefrac_l, cdist_l (nx+2*halo_i, ny+2*halo_j) of the open coast', 1_c_int)
    call ensure_ctx()
    rc = c_um_ice(ctx, landfrac_l, icefrac_l, cdist_l)
    if (rc /= 0) call fail('um_ice', rc)
  end subroutine um_ice

  subroutine um_ice_dev(landfrac_l, icefrac_l, cdist_l)
    type(c_ptr), intent(in) :: landfrac_l, icefrac_l, cdist_l
    integer(c_int) :: rc
    call ensure_ctx()
    rc = c_um_ice_dev(ctx, landfrac_l, icefrac_l, cdist_l, c_null_ptr)
    if (rc /= 0) call fail('um_ice_dev', rc)
  end subroutine um_ice_dev

  ! (synchronises) calls since the open / those after the first whose coast differed (-1: every call computes the whole
  ! interior) / workgroup tiles (4 rows x 64 columns) the last call marked / tiles of the grid
  subroutine um_ice_report(rep)
    integer(c_long_long), intent(out) :: rep(4)
    integer(c_int) :: rc
    call ensure_ctx()
    rep = 0
    rc = c_um_ice_report(ctx, rep)
    if (rc /= 0) call fail('um_ice_report', rc)
  end subroutine um_ice_report

  subroutine um_coast_close()
    integer(c_int) :: rc
    call ensure_ctx()
    rc = c_um_coast_close(ctx)
    if (rc /= 0) call fail('um_coast_close', rc)
    um_shape = 0
  end subroutine um_coast_close

  !---------------------------------------------------------------------------
  ! One tile of the UM's 2-D decomposition whose coast moves with the sea ice (include/seabreeze_hip.h:
  ! sb_um_tile_coast_open): what a UM rank calls, because um_ice keeps the interior-only rule and its field depends on the
  ! cut.  Open once per landfrac -- true_latitude_l, true_longitude_l on tdims_l (nx+2*halo_i, ny+2*halo_j), degrees, ghost
  ! cells filled, are copied; beyond(4): the domain's cells beyond the tile's west, east, south and north side (0: the
  ! domain's edge); the window is +-win_i x +-win_j, each 0 .. 255; every side needs a halo of min(window, beyond) + 1 --
  ! then, per timestep, one swap_bounds of icefrac_l and um_tile_ice: landfrac_l, icefrac_l and cdist_l on tdims_l.  Only
  ! the interior of cdist_l is written -- the tile's cells of the whole-domain field -- and what a call left there must
  ! still be there at the next one.  um_tile_ice_dev takes device frames and only enqueues on the context's stream.
  !---------------------------------------------------------------------------
  subroutine um_tile_coast_open(true_latitude_l, true_longitude_l, halo_i, halo_j, win_i, win_j, beyond, maxdist, incremental)
    real, intent(in), contiguous :: true_latitude_l(:,:), true_longitude_l(:,:)
    integer, intent(in) :: halo_i, halo_j, win_i, win_j, beyond(4)
    real, intent(in), optional :: maxdist
    logical, intent(in), optional :: incremental
    real :: md
    integer(c_int) :: rc, inc, nx, ny
    if (any(shape(true_longitude_l) /= shape(true_latitude_l))) &
      call fail('um_tile_coast_open: need true_latitude_l, true_longitude_l (nx+2*halo_i, ny+2*halo_j)', 1_c_int)
    nx = int(size(true_latitude_l, 1) - 2*halo_i, c_int); ny = int(size(true_latitude_l, 2) - 2*halo_j, c_int)
    md = 180.
    if (present(maxdist)) md = maxdist
    inc = 1_c_int
    if (present(incremental)) inc = merge(1_c_int, 0_c_int, incremental)
    call ensure_ctx()
    rc = c_um_tile_coast_open(ctx, nx, ny, int(halo_i, c_int), int(halo_j, c_int), int(win_i, c_int), int(win_j, c_int), &
                              int(beyond, c_int), true_latitude_l, true_longitude_l, real(md, rk), inc)
    if (rc /= 0) call fail('um_tile_coast_open', rc)
    um_tile_shape = [nx, ny, int(halo_i, c_int), int(halo_j, c_int)]
  end subroutine um_tile_coast_open

  subroutine um_tile_ice(landfrac_l, icefrac_l, cdist_l)
    real, intent(in), contiguous :: landfrac_l(:,:), icefrac_l(:,:)
    real, intent(inout), contiguous :: cdist_l(:,:)
    integer(c_int) :: rc
    integer :: want(2)
    want = [um_tile_shape(1) + 2*um_tile_shape(3), um_tile_shape(2) + 2*um_tile_shape(4)]
    if (um_tile_shape(1) < 1) call fail('um_tile_ice without um_tile_coast_open', 1_c_int)
    if (any(shape(landfrac_l) /= want) .or. any(shape(icefrac_l) /= want) .or. any(shape(cdist_l) /= want)) &
      call fail('um_tile_ice: need landfrac_l, icefrac_l, cdist_l (nx+2*halo_i, ny+2*halo_j) of the open coast', 1_c_int)
    call ensure_ctx()
    rc = c_um_tile_ice(ctx, landfrac_l, icefrac_l, cdist_l)
    if (rc /= 0) call fail('um_tile_ice', rc)
  end subroutine um_tile_ice

  subroutine um_tile_ice_dev(landfrac_l, icefrac_l, cdist_l)
    type(c_ptr), intent(in) :: landfrac_l, icefrac_l, cdist_l
    integer(c_int) :: rc
    call ensure_ctx()
    rc = c_um_tile_ice_dev(ctx, landfrac_l, icefrac_l, cdist_l, c_null_ptr)
    if (rc /= 0) call fail('um_tile_ice_dev', rc)
  end subroutine um_tile_ice_dev

  ! (synchronises) um_ice_report's four fields for the tile coast
  subroutine um_tile_ice_report(rep)
    integer(c_long_long), intent(out) :: rep(4)
    integer(c_int) :: rc
    call ensure_ctx()
    rep = 0
    rc = c_um_tile_ice_report(ctx, rep)
    if (rc /= 0) call fail('um_tile_ice_report', rc)
  end subroutine um_tile_ice_report

  subroutine um_tile_coast_close()
    integer(c_int) :: rc
    call ensure_ctx()
    rc = c_um_tile_coast_close(ctx)
    if (rc /= 0) call fail('um_tile_coast_close', rc)
    um_tile_shape = 0
  end subroutine um_tile_coast_close

  !---------------------------------------------------------------------------
  ! ref: generic/sea_breeze_diag.f90:457-481
  !---------------------------------------------------------------------------
  subroutine sigmoid(ary, sm)
    real, intent(in), contiguous :: ary(:,:)
    real, intent(out), contiguous :: sm(:,:)
    integer(c_int) :: rc
    if (any(shape(sm) /= shape(ary))) call fail('sigmoid: shape mismatch', 1_c_int)
    call ensure_ctx()
    rc = c_sigmoid(ctx, int(size(ary, 1), c_int), int(size(ary, 2), c_int), ary, sm)
    if (rc /= 0) call fail('sigmoid', rc)
  end subroutine sigmoid

end module sea_breeze_diag_mod
